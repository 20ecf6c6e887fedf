"""The BAM that `mapad-amd map` writes, record by record against the oracle's own search and records (tests/cli_audit_util.py; CPU twin: tests/test_cli_audit_host.py):
world A of records_util indexed on disk, 2540 mappable reads with random input flags and tags, 300 of them byte-identical copies, three records that cannot be mapped —
through one chunk, many chunks, two workers, coalesced launches, collapsed duplicates, the host's text path, uploaded hits, FASTQ input and every opt-in accumulator.
Every run is one child process under a time limit of its own; once a child has died no further one is started."""
import os
import subprocess

import pytest

import cli_audit_util as au
from bam_util import read_bam

pytestmark = pytest.mark.gpu

_died = []  # the first child that failed or ran into its time limit


def _child(cmd, env=None):
    if _died:
        pytest.fail(f"not started: an earlier child died ({_died[0]})")
    try:
        subprocess.check_call(["timeout", "-k", "10", "300"] + cmd, env=env)
    except subprocess.CalledProcessError as e:
        _died.append(f"exit status {e.returncode}: {' '.join(cmd[:8])} ...")
        raise


@pytest.fixture(scope="module")
def audit(tmp_path_factory):
    d = tmp_path_factory.mktemp("cli_audit")
    fa = str(d / "ref.fa")
    world, clean = au.indexed_world(fa, run=_child)
    recs = au.audit_input(world, clean)
    expect = {}

    def expectation(preset):
        if preset not in expect:
            au.check_cli_flags_are_the_preset(preset)
            expect[preset] = au.expectation(world, preset, recs)
        return expect[preset]
    expectation("damage")  # once, here: eleven of the twelve runs share it
    return dict(dir=str(d), fa=fa, world=world, recs=recs, files=au.write_inputs(str(d), recs), expectation=expectation)


# id -> (input form, preset, extra arguments ("F": a file of the run's own), extra environment)
VARIANTS = {
    "one_chunk": ("bam", "damage", ["--batch_size", "250000"], {}),
    "chunks": ("bam", "damage", ["--batch_size", "301"], {}),  # 4 in flight
    "serial": ("bam", "damage", ["--batch_size", "301", "--in_flight", "1"], {}),
    "two_devices_deep": ("bam", "damage", ["--devices", "0,0", "--batch_size", "301", "--in_flight", "7"], {}),
    "coalesced": ("bam", "damage", ["--batch_size", "97", "--coalesce", "3", "--coalesce_steady", "5"], {}),
    "collapsed": ("bam", "damage", ["--batch_size", "301", "--collapse_duplicates"], {}),
    "text_on_host": ("bam", "damage", ["--batch_size", "301"], {"MAPAD_RECORDS_TEXT": "host"}),
    "uploaded": ("bam", "damage", ["--batch_size", "301"], {"MAPAD_RECORDS_RESIDENT": "0"}),
    "fastq": ("fastq", "damage", ["--batch_size", "301"], {}),
    "fastq_gz": ("fastq_gz", "damage", ["--batch_size", "301"], {}),
    "no_damage": ("bam", "no_damage", ["--batch_size", "301"], {}),
    "everything_on": ("bam", "damage", ["--batch_size", "301", "--mark_duplicates", "--damage_score", "--damage_profile", "F", "--coverage", "F", "--pileup", "F",
                                        "--allele_likelihoods", "F", "--genotype_vcf", "F"], {}),
}


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_written_bam_equals_the_oracles_records(audit, variant):
    form, preset, extra, env = VARIANTS[variant]
    recs = audit["recs"] if form == "bam" else au.as_fastq(audit["recs"])
    rows = au.rows_by_input(recs, audit["expectation"](preset)[0 if form == "bam" else 1])
    out = os.path.join(audit["dir"], variant + ".bam")
    extra = [os.path.join(audit["dir"], f"{variant}.{extra[i - 1][2:]}") if a == "F" else a for i, a in enumerate(extra)]
    _child([au.cli(), "--seed", str(au.SEED), "map", "-r", audit["files"][form], "-g", audit["fa"], "-o", out] + au.cli_flags(preset) + extra, env=dict(os.environ, **env))
    _, refs, got = read_bam(out)
    assert refs == au.header_refs(audit["world"])
    everything = variant == "everything_on"
    n_bad, first, per_field = au.compare(got, rows, recs, **(dict(flag_mask=0xFFFF & ~0x400, drop_tags=("DS",)) if everything else {}))
    print(variant, len(got), "records compared,", n_bad, "differ")
    assert n_bad == 0, au.report(len(got), n_bad, first, per_field, variant)
    if everything:
        # 0x400 from the input passes through; it is added exactly where (tid, POS, span, strand) repeats an earlier record of the expectation
        want = au.expected_duplicates(rows)
        wrong = [(i, r["name"]) for i, (g, r, w) in enumerate(zip(got, recs, want)) if bool(g["flags"] & 0x400) != (w or bool(r["flags"] & 0x400))]
        print(variant, sum(want), "duplicates expected")
        assert sum(want) >= 50 and not wrong, wrong[:10]  # (the expectation holds 108 such records: a condition at half of the yield)
    if variant == "one_chunk":  # the reach conditions on what the BAM says
        counts = au.reach_counts([au.view_of_bam(g) for g in got], recs)
        print(variant, counts)
        au.check_reach(counts)
