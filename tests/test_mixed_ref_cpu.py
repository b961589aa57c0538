"""tests/mixed_ref.py on the CPU, with the oracle alone: every chunk of the inputs the failed-chunk tests draw
from has a failing flip that leaves every other chunk as it was, and the stages' references accept the empty
chunks that stand for failed ones."""
import numpy as np
import pytest

from oracle import oracle as O
import mixed_ref as M
import seqpack_ref as R
from stage_rig import references


@pytest.mark.parametrize("name,nchunks", [("l6_c20", 8), ("huffonly_c20", 14), ("memlevel1_c10", 148)])
def test_every_chunk_has_a_failing_flip(name, nchunks):
    gz, cs = R.load_input(name)
    oi = O.build_index(gz, cs)
    assert oi.count - 1 == nchunks
    clean = [O.extract(gz, oi, j) for j in range(nchunks)]
    for k in range(nchunks):
        bad, code = M.corrupt_chunk(gz, oi, k, clean)       # (asserts every other chunk's text unchanged)
        assert code == -3 and len(bad) == len(gz)
        diff = np.flatnonzero(np.frombuffer(bad, np.uint8) != np.frombuffer(gz, np.uint8))
        i0, i1 = oi.point(k)[1], oi.point(k + 1)[1]
        assert diff.size == 6 and i0 + 8 <= diff[0] and diff[-1] < i1 - 2 and (diff[0] - i0 - 8) % 37 == 0


@pytest.mark.parametrize("name,failed", M.CASES + ((M.L6, tuple(range(8))),))
def test_references_accept_empty_chunks(name, failed):
    """The mixed reference is the reference of the good chunks alone, with a 0 at every failed chunk."""
    bad, cs, codes, mixed, clean = M.mixed_input(name, failed)
    assert set(codes) == set(failed) and set(codes.values()) == {-3}
    good = tuple(c for k, c in enumerate(clean) if k not in failed)
    a, b = references(mixed, strict=False), references(good, strict=False)
    keep = np.array([k not in failed for k in range(len(clean))])
    assert a["query"]["records"] == sum(len(c[2]) for c in good)
    for stage, key in (("query", "chunk_hits"), ("filter", "chunk_passed"), ("trim", "chunk_kept"), ("dedup", "chunk_unique"),
                       ("profile", "chunk_profiled")):
        assert np.array_equal(a[stage][key][keep], b[stage][key]) and not a[stage][key][~keep].any(), (stage, key)
    for stage, keys in (("pack", ("seq_off", "seq_len", "bases", "mask")), ("query", ("hits", "mask", "counts")),
                        ("filter", ("passed", "mask", "metrics")), ("trim", ("kept", "rows", "mask")),
                        ("dedup", ("unique", "first", "table", "mask", "level_reads")), ("profile", ("profiled", "table", "gc_hist")),
                        ("select", ("recno", "sel_off", "desc", "bytes"))):
        for key in keys:
            assert np.array_equal(a[stage][key], b[stage][key]), (stage, key)


def test_cut_range():
    part, cs, codes, mixed = M.cut_input()
    gz, _ = R.load_input(M.CUT[0])
    oi = O.build_index(gz, cs)
    lo, hi = M.comp_bounds(oi, 0, M.CUT[1])
    assert part == gz[lo:hi - M.CUT[2]] and codes == {M.CUT[1] - 1: -3}
    assert [len(c[2]) for c in mixed[:-1]] == [len(c[2]) for c in R.oracle_chunks(M.CUT[0])[:M.CUT[1] - 1]] and len(mixed[-1][2]) == 0
    # the whole range still decodes
    assert M.extract_until(gz, oi, M.CUT[1] - 1, hi) == O.extract(gz, oi, M.CUT[1] - 1)
