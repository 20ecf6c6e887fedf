"""The audit of tests/cli_audit_util.py without a GPU: the run's mappable reads cut into the slices `mapad-amd map --batch_size 301 --devices 0,0` makes, each slice
mapped by the host build of the kernels' per-read logic (tests/emu) and turned into records by the host path seeded with mapad_records_seed_at(0, first_read + lo), against
the oracle's own search and records of the whole run as one batch.  Pins the seed arithmetic and the flag rule to the oracle, and proves the reach conditions of the table
that tests/test_gpu_cli_audit.py holds the written BAM to.  Tag order, bin and the records that cannot be mapped are the writer's: GPU side only."""
import subprocess

import numpy as np
import pytest

import mapad_amd

import cli_audit_util as au
import emu_util
import records_util as ru
from bam_util import read_bam

PRESET = "damage"


@pytest.fixture(scope="module")
def audit(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_audit_host")
    world, clean = au.indexed_world(str(d / "ref.fa"))
    recs = au.audit_input(world, clean)
    return world, recs, au.expectation(world, PRESET, recs)


def test_cli_flags_are_the_presets():
    for preset in au.CLI_PRESETS:
        au.check_cli_flags_are_the_preset(preset)


def test_expectation_reaches_what_the_audit_is_for(audit):
    world, recs, (rows, rows_fq) = audit
    counts = au.reach_counts([None if r is None else au.view_of_row(r) for r in au.rows_by_input(recs, rows)], recs)
    print(PRESET, counts)
    au.check_reach(counts)
    assert [(n, s, e - s + 1) for n, s, e in world.pidx.contigs()] == [(n, int(world.starts[k]), ln) for k, (n, ln) in enumerate(au.header_refs(world))]


@pytest.fixture(scope="module")
def searched(audit):
    """the slices of `--batch_size 301 --devices 0,0`, each with its reads and the host emulation's hits (the search sees neither flags nor tags: one run serves both forms)"""
    world, recs, _ = audit
    seqs, quals, offsets = au.mappable_batch(recs)
    slices = au.cli_slices(recs, 301, 2)
    assert len(slices) >= 16 and any(hi - lo != slices[0][2] - slices[0][1] for _, lo, hi in slices)  # many chunks, of uneven size around the records that cannot be mapped
    out = []
    for first, lo, hi in slices:
        a, b = first + lo, first + hi
        batch = (seqs[int(offsets[a]):int(offsets[b])], quals[int(offsets[a]):int(offsets[b])], offsets[a:b + 1] - offsets[a])
        out.append((a, b, batch, emu_util.map_batch(world.pidx, ru.params(PRESET), *batch)))
    assert out[-1][1] == len(offsets) - 1
    return out


@pytest.mark.parametrize("form", ["bam", "fastq"])
def test_host_path_in_the_command_lines_slices_equals_the_oracle(audit, searched, form):
    world, recs, (rows, rows_fq) = audit
    inputs, rows = (recs, rows) if form == "bam" else (au.as_fastq(recs), rows_fq)
    m = [r for r in inputs if r["mappable"]]
    got = []
    for a, b, batch, res in searched:
        out = mapad_amd.hits_to_records(world.pidx, ru.params(PRESET), res, *batch, in_flags=np.array([r["flags"] for r in m[a:b]], np.uint16),
                                        seed=int(mapad_amd.lib().mapad_records_seed_at(au.SEED, a)))
        got += [au.host_record(r, inp) for r, inp in zip(out, m[a:b])]
    n_bad, first, per_field = au.compare(got, rows, m)
    print(form, len(got), "records compared,", n_bad, "differ")
    assert n_bad == 0, au.report(len(got), n_bad, first, per_field, form)


def test_recoded_input_files_hold_what_the_comparison_expects_of_unmapped_records(audit, tmp_path):
    """`mapad-amd recode` (reader and writer without a search) over the three input files: every record comes back under the rule for unmapped records — flags, SEQ and
    QUAL un-reversed, surviving input tags in input order, then XD, bin 4680 — which is also what the comparison holds the records that cannot be mapped to on the GPU."""
    _, recs, _ = audit
    for form, path in au.write_inputs(str(tmp_path), recs).items():
        out = str(tmp_path / (form + ".out.bam"))
        subprocess.check_call([au.cli(), "recode", "-r", path, "-o", out], stderr=subprocess.DEVNULL)
        inputs = recs if form == "bam" else au.as_fastq(recs)
        got = read_bam(out)[2]
        n_bad, first, per_field = au.compare(got, [None] * len(inputs), inputs)
        assert n_bad == 0, au.report(len(got), n_bad, first, per_field, form)
    assert sum(bool(r["tags"]) for r in recs) > 1000 and sum(r["flags"] & 0x10 == 0x10 for r in recs) > 400
