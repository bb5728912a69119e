"""jspb_expand_lines, the host's expansion of the compaction service's bitmap
answer (svc_wait_bits and the host lease share it), against a
numpy reference. A pure host function: no engine, no GPU.

A line is 8 words: tile t's 256 leaf bits as four 64-bit words, each stored as
two halves (seq << 32 | 32 bits), low half first. Job j gets the j-th set bit
in tile order, as base + l0[t] + bit index."""
import ctypes

import numpy as np
import pytest

from jobset_amd import native

SEQ = 0x1234567
BASE = 7
TILES = [1, 2, 8, 9, 15]


def pack(bits: np.ndarray, seq: int = SEQ) -> np.ndarray:
    """[tiles, 256] bools -> [tiles, 8] u64 tagged halves."""
    n = bits.shape[0]
    w = np.packbits(bits.reshape(n, 8, 32), axis=2, bitorder="little").view("<u4").reshape(n, 8)
    return (np.uint64(seq) << np.uint64(32)) | w.astype(np.uint64)


def reference(bits: np.ndarray, l0: np.ndarray, J: int, upto: int = None):
    """(assign[J], placed) from the first `upto` lines (all by default)."""
    t, i = np.nonzero(bits[:upto])
    leaves = (BASE + l0[t] + i).astype(np.int32)[:J]
    out = np.full(J, -1, dtype=np.int32)
    out[:leaves.size] = leaves
    return out, int(leaves.size)


def expand(lines: np.ndarray, l0: np.ndarray, J: int, seq: int = SEQ):
    out = np.full(J + 4, -7, dtype=np.int32)  # -7: never written
    placed = ctypes.c_uint32(0xFFFFFFFF)
    lines = np.ascontiguousarray(lines, dtype=np.uint64)
    l0 = np.ascontiguousarray(l0, dtype=np.uint32)
    rc = native.lib().jspb_expand_lines(lines.ctypes.data, lines.shape[0], l0.ctypes.data, BASE, seq, J,
                                        out.ctypes.data, ctypes.byref(placed))
    return rc, out, placed.value


def patterns(n: int):
    rng = np.random.default_rng(100 + n)
    ones = np.ones((n, 256), dtype=bool)
    zeros = np.zeros((n, 256), dtype=bool)
    bit0, bit63 = zeros.copy(), zeros.copy()
    bit0[:, 0] = True
    bit63[:, 63] = True
    bit63[n - 1, 255] = True
    # runs across the 32-bit halves and the 64-bit words, one ending a line
    runs = zeros.copy()
    for a, b in ((20, 45), (50, 80), (120, 200), (250, 256)):
        runs[:, a:b] = True
    runs[::2, 31:33] = True
    # cfg2's shape: 68 leaves per tile, a few infeasible
    racks = zeros.copy()
    racks[:, :68] = rng.random((n, 68)) > 0.03
    return {"ones": ones, "zeros": zeros, "bit0": bit0, "bit63": bit63, "runs": runs, "racks": racks,
            "random": rng.random((n, 256)) > 0.5, "sparse": rng.random((n, 256)) > 0.97}


@pytest.mark.parametrize("n", TILES)
def test_expansion_equals_reference(n):
    for name, bits in patterns(n).items():
        l0 = np.arange(n, dtype=np.uint32) * (68 if name == "racks" else 256)
        lines = pack(bits)
        feasible = int(bits.sum())
        for J in sorted({0, 1, feasible, max(feasible - 1, 0), feasible + 5}):
            rc, out, placed = expand(lines, l0, J)
            want, n_want = reference(bits, l0, J)
            assert rc == 0, (name, J)
            assert placed == n_want == min(J, feasible), (name, J)
            np.testing.assert_array_equal(out[:J], want, err_msg=f"{name} J={J}")
            assert (out[J:] == -7).all(), (name, J)


@pytest.mark.parametrize("n", TILES)
def test_wrong_tag_stops_at_the_last_whole_line(n):
    bits = patterns(n)["racks"]
    l0 = np.arange(n, dtype=np.uint32) * 68
    feasible = int(bits.sum())
    for bad_line in sorted({0, n // 2, n - 1}):
        for half in (0, 3, 7):
            lines = pack(bits)
            lines[bad_line, half] = (np.uint64(SEQ + 1) << np.uint64(32)) | (lines[bad_line, half] & np.uint64(0xFFFFFFFF))
            before = int(bits[:bad_line].sum())
            # more jobs than the whole lines hold: the mismatch is reported,
            # the whole lines' jobs stand, nothing else is written (no -1 tail)
            for J in (before + 1, feasible, feasible + 5):
                rc, out, placed = expand(lines, l0, J)
                assert rc == 1 and placed == before, (bad_line, half, J)
                np.testing.assert_array_equal(out[:before], reference(bits, l0, J, upto=bad_line)[0][:before])
                assert (out[before:] == -7).all(), (bad_line, half, J)
            # jobs the whole lines before it satisfy: that line is never read
            if before > 0:
                rc, out, placed = expand(lines, l0, before)
                assert rc == 0 and placed == before
                np.testing.assert_array_equal(out[:before], reference(bits, l0, before)[0])


def test_another_request_number_matches_nothing():
    bits = patterns(2)["ones"]
    rc, out, placed = expand(pack(bits), np.array([0, 256], dtype=np.uint32), 10, seq=SEQ + 1)
    assert rc == 1 and placed == 0 and (out == -7).all()
    rc, out, placed = expand(pack(bits), np.array([0, 256], dtype=np.uint32), 0, seq=SEQ + 1)
    assert rc == 0 and placed == 0  # no job: no line is needed
