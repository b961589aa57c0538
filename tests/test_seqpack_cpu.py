"""Packed reads on the CPU: the numpy reference of the format (tests/seqpack_ref.py) read back
through PackedReads.sequence / .quality against the oracle's Sequence / Quality slices, a guard
that the inputs of the GPU test cover every path of the pack kernel, and the argument errors that
need no device."""
import ctypes as C

import numpy as np
import pytest

import parallelparsing_amd as pp
from parallelparsing_amd import _lib
import seqpack_ref as R


def host_packed(ref):
    return pp.PackedReads(ref["seq_off"], ref["seq_len"], ref["bases"], ref["mask"], ref["qual"])


@pytest.mark.parametrize("name", R.ALL_INPUTS)
def test_reference_reads_back_as_the_oracle_slices(name):
    """sequence(j) == the Sequence slice [n1+1, n2) with every non-ACGT byte as 'N'; quality(j) == the
    Quality slice [n3+1, n4) cut or zero-filled to L_j."""
    ref = R.reference(name)
    pk = host_packed(ref)
    keep = np.frombuffer(b"ACGT", np.uint8)
    j = 0
    for _, raw, desc in R.oracle_chunks(name):
        r = np.frombuffer(raw, np.uint8)
        for n1, n2, n3, n4 in desc.astype(np.int64):
            seq = r[n1 + 1:n2].copy()
            seq[~np.isin(seq, keep)] = ord("N")
            assert pk.sequence(j) == seq.tobytes(), (name, j)
            L = int(n2 - n1 - 1)
            q = r[n3 + 1:n4][:L].tobytes()
            assert pk.quality(j) == q + b"\0" * (L - len(q)), (name, j)
            assert int(ref["seq_off"][j]) % 32 == 0 and int(ref["seq_len"][j]) == L
            j += 1
    assert j == pk.records == ref["seq_len"].size
    assert ref["bases"].size * 16 == ref["mask"].size * 32 == ref["qual"].size == int(ref["seq_off"][-1])


def test_gpu_inputs_cover_every_path():
    """Over the inputs tests/test_gpu_seqpack.py packs, the reference must find: all 32 residues of
    L mod 32 (a non-empty multiple of 32 among them), an empty sequence, masked bases, a sequence
    straddling offset_k and the body, one wholly inside offset_k, a record whose quality length
    differs from L, and a record the reference parses twice."""
    residues, nonempty32, empty, masked = set(), 0, 0, 0
    straddle, in_carry, qdiff, q1 = 0, 0, 0, 0
    for name in R.ALL_INPUTS:
        ref = R.reference(name)
        L = ref["seq_len"].astype(np.int64)
        residues |= set((L % 32).tolist())
        nonempty32 += int(((L % 32 == 0) & (L > 0)).sum())
        empty += int((L == 0).sum())
        masked += int(sum(bin(int(w)).count("1") for w in ref["mask"]))
        for off, _, desc in R.oracle_chunks(name):
            d = desc.astype(np.int64)
            if not len(d):
                continue
            n1, n2, n3, n4 = d[:, 0], d[:, 1], d[:, 2], d[:, 3]
            olen = len(off)
            nonz = n2 - n1 - 1 > 0
            straddle += int((nonz & (n1 + 1 < olen) & (n2 > olen)).sum())
            in_carry += int((nonz & (n2 <= olen)).sum())
            qdiff += int(((n4 - n3 - 1) != (n2 - n1 - 1)).sum())
            q1 += int(d[0, 3] < olen)      # the chunk's first record ends inside the carry: parsed twice
    assert residues == set(range(32)), sorted(set(range(32)) - residues)
    assert nonempty32 > 0 and empty > 0 and masked > 0
    assert straddle > 0 and in_carry > 0 and qdiff > 0 and q1 > 0


def test_synthetic_input_is_the_one_the_issue_measured():
    """23 chunks, 2,997 parsed records, all residues, 456 non-empty multiples of 32, 33,755 masked
    bases, 4 straddling and 8 in-carry sequences."""
    ch = R.oracle_chunks(R.SYNTH)
    ref = R.reference(R.SYNTH)
    L = ref["seq_len"].astype(np.int64)
    assert len(ch) == 23 and L.size == 2997
    assert set((L % 32).tolist()) == set(range(32))
    assert int(((L % 32 == 0) & (L > 0)).sum()) == 456
    assert sum(bin(int(w)).count("1") for w in ref["mask"]) == 33755
    straddle = in_carry = 0
    for off, _, desc in ch:
        d = desc.astype(np.int64)
        nonz = d[:, 1] - d[:, 0] - 1 > 0
        straddle += int((nonz & (d[:, 0] + 1 < len(off)) & (d[:, 1] > len(off))).sum())
        in_carry += int((nonz & (d[:, 1] <= len(off))).sum())
    assert (straddle, in_carry) == (4, 8)


def test_null_handles_are_argument_errors():
    """Every new entry point with a NULL handle returns PPG_ARG_ERROR (no device needed)."""
    lib, E = _lib.lib, _lib.PPG_ARG_ERROR
    v = C.c_int64()
    h = C.c_void_p()
    buf = np.zeros(64, np.int64)
    p = C.c_void_p(buf.ctypes.data)
    assert lib.ppg_shard_seq_bases(None, C.byref(v), C.byref(v)) == E
    assert lib.ppg_shard_pack_seq(None, p, p, 1, p, p, p, 32, C.byref(v)) == E
    assert lib.ppg_shard_set_seqpack(None, p, p, 1, p, p, p, 32) == E
    assert lib.ppg_shard_set_seqpack(None, None, None, 0, None, None, None, 0) == E
    assert lib.ppg_shard_seqpack_ready(None, C.byref(v)) == E
    assert lib.ppg_cursor_open_packed(None, None, b"x.gz", 0, 0, 0, 1, 1, C.byref(h)) == E
    assert not h.value
    assert lib.ppg_cursor_packed(None, C.byref(h), C.byref(h), C.byref(h), C.byref(h), C.byref(v)) == E
    assert lib.ppg_cursor_packed_offsets(None, p, 64) == E


def test_packed_reads_host_container():
    """PackedReads.empty on the host: plane sizes, base_cap rounded to a unit, no quality plane."""
    pk = pp.PackedReads.empty(3, 70, quality=False)
    assert (pk.rec_cap, pk.base_cap) == (3, 96) and pk.qual is None and not pk.on_device
    assert pk.seq_off.size == 4 and pk.bases.size == 6 and pk.mask.size == 3
    assert pk.to_host() is pk
    with pytest.raises(ValueError):
        pk.quality(0)
