"""The host index build (SA-IS, mapad_index_build) against the numpy restatement of the index products in tests/index_util.py — the reference that
tests/test_gpu_index_chunks.py holds the GPU builder to — on the texts the two files share, and the restatement itself against the oracle's naive suffix sort
where that one is usable.  No GPU needed."""
import numpy as np
import pytest

import mapad_amd
from oracle import binding as ob

import index_util as iu

NAMES = ["mixed", "two_copies_20k", "n_runs", "polyA", "tandem", "uniform3", "uniform9", "uniform257", "uniform4097"]


@pytest.mark.parametrize("name", NAMES)
def test_host_index_equals_numpy_reference(name):
    contigs, ref = iu.contigs(name), iu.reference(name)
    ix = mapad_amd.Index.build(contigs)
    iu.assert_index_equals_reference(ix, ref, name)  # incl. sa_get_batch over all rows: the LF walk over the rank blocks, independent of how they were built
    if ref.n <= 20_000:  # the oracle sorts suffixes by comparing them: unusable on the long periodic texts
        text = b"".join(s for _, s in contigs).upper().replace(b"N", b"X")
        o = ob.OracleIndex.from_text(text, "$ACGTX", 128)
        assert np.array_equal(o.sa(), ref.sa)
        assert np.array_equal(o.bwt(), ref.bwt)


def test_last_build_info_surface():
    """The info call of the GPU builder exists, refuses a null pointer and reports nothing for host builds (they do not go through the doubling loop)."""
    assert mapad_amd.lib().mapad_last_index_build_info(None) == -1
    before = mapad_amd.Index.last_build_info()
    assert list(before) == ["rounds", "unresolved", "chunks", "cut_last_head", "cut_first_head", "tails", "whole", "largest_chunk", "pieces", "chunk_limit", "sort_cap"]
    mapad_amd.Index.build(iu.contigs("uniform257"))
    assert mapad_amd.Index.last_build_info() == before


def test_rank_text_and_suffix_array_on_a_worked_example():
    """ACNNNNNNNNNNNNNNNNNNNNG (20 N) by hand: ranks, the reverse complement with X kept, and the suffix order checked by comparing suffixes directly."""
    t = iu.rank_text([("a", b"ac"), ("b", b"N" * 20 + b"g")])
    assert t.tolist() == [1, 2] + [5] * 20 + [3, 0, 2] + [5] * 20 + [3, 4, 0]
    sa = iu.suffix_array(t).tolist()
    tb = bytes(t)
    assert sa == sorted(range(len(t)), key=lambda i: tb[i:])  # a shorter suffix that is a prefix of a longer one sorts first, as bytes do
