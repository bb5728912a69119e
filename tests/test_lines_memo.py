"""The host functions behind the lease's kept list ("the kept
list"): jspb_list_answer, the answer for J jobs copied from a list of feasible
leaves that jspb_expand_lines decoded once, against a fresh jspb_expand_lines
of the same lines; and jspb_lines_tagged, the tag check every such answer
makes. Pure host functions: no engine, no GPU. The lines are those of
test_expand_lines.py (its patterns and its pack)."""
import ctypes

import numpy as np
import pytest

from jobset_amd import native
from test_expand_lines import SEQ, TILES, expand, pack, patterns


def list_answer(lst: np.ndarray, n_list: int, J: int):
    out = np.full(J + 4, -7, dtype=np.int32)  # -7: never written
    placed = ctypes.c_uint32(0xFFFFFFFF)
    lst = np.ascontiguousarray(lst, dtype=np.int32)
    rc = native.lib().jspb_list_answer(lst.ctypes.data, n_list, J, out.ctypes.data, ctypes.byref(placed))
    assert rc == 0
    return out, placed.value


def tagged(lines: np.ndarray, n_tiles: int, seq: int = SEQ) -> int:
    lines = np.ascontiguousarray(lines, dtype=np.uint64)
    return native.lib().jspb_lines_tagged(lines.ctypes.data, n_tiles, seq)


def cases(n):
    for name, bits in patterns(n).items():
        l0 = np.arange(n, dtype=np.uint32) * (68 if name == "racks" else 256)
        yield name, bits, l0, pack(bits), int(bits.sum())


@pytest.mark.parametrize("n", TILES)
def test_answer_from_the_whole_list_equals_a_fresh_expansion(n):
    for name, bits, l0, lines, nF in cases(n):
        rc, lst, n_list = expand(lines, l0, 256 * n)
        assert rc == 0 and n_list == nF, name
        for J in sorted({J for J in (1, nF - 1, nF, nF + 1, 256 * n) if J >= 1}):
            rc, want, want_placed = expand(lines, l0, J)
            assert rc == 0, (name, J)
            got, placed = list_answer(lst[:256 * n], n_list, J)
            assert placed == want_placed == min(J, nF), (name, J)
            np.testing.assert_array_equal(got[:J], want[:J], err_msg=f"{name} J={J}")
            assert (got[J:] == -7).all(), (name, J)  # nothing behind out[J - 1]


@pytest.mark.parametrize("n", TILES)
def test_answer_from_a_short_list(n):
    """A list built for J_b < nF jobs answers every J <= J_b as a fresh
    expansion does."""
    for name, bits, l0, lines, nF in cases(n):
        for J_b in sorted({J for J in (1, nF // 2, nF - 1) if 1 <= J < nF}):
            rc, lst, n_list = expand(lines, l0, J_b)
            assert rc == 0 and n_list == J_b, (name, J_b)
            for J in sorted({1, max(J_b // 2, 1), max(J_b - 1, 1), J_b}):
                rc, want, want_placed = expand(lines, l0, J)
                got, placed = list_answer(lst[:J_b], n_list, J)
                assert rc == 0 and placed == want_placed == J, (name, J_b, J)
                np.testing.assert_array_equal(got[:J], want[:J], err_msg=f"{name} J_b={J_b} J={J}")
                assert (got[J:] == -7).all(), (name, J_b, J)


def test_empty_list_and_no_jobs():
    got, placed = list_answer(np.zeros(1, dtype=np.int32), 0, 3)
    assert placed == 0 and (got[:3] == -1).all() and (got[3:] == -7).all()
    got, placed = list_answer(np.arange(5, dtype=np.int32), 5, 0)
    assert placed == 0 and (got == -7).all()


@pytest.mark.parametrize("n", [1, 15])
def test_tag_check_sees_every_half(n):
    bits = patterns(n)["racks"]
    lines = pack(bits)
    assert tagged(lines, n) == 1
    assert tagged(lines, n, SEQ + 1) == 0
    assert tagged(lines, 0) == 1  # no line: nothing to check
    for t in range(n):
        for half in range(8):
            for other in (SEQ + 1, SEQ ^ 0x80000000, 0):
                bad = lines.copy()
                bad[t, half] = (np.uint64(other) << np.uint64(32)) | (bad[t, half] & np.uint64(0xFFFFFFFF))
                assert tagged(bad, n) == 0, (t, half, other)
                # only the first k lines are read
                for k in sorted({0, t, t + 1, n}):
                    assert tagged(bad, k) == (1 if k <= t else 0), (t, half, k)
