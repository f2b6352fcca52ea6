"""CPU checks of the fused plain view (csrc/nce_common.h: FusedLayout, ViewLayout) through
rsx_nce_fused_workspace_floats, rsx_nce_view_ints and rsx_nce_view_fill_host. The library loads
without a GPU (tests/test_native_abi.py)."""
import ctypes
import os
import struct

import pytest

import recsys_amd  # noqa: F401
from recsys_amd import _native

SIZES = (0, 1, 127, 128, 129, 1029, 5000)
ONE = struct.unpack("<i", struct.pack("<f", 1.0))[0]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load()


def _regions(lib, n, m):
    """[begin, end) float ranges of the fused workspace, rebuilt from the documented layout: the
    grouped layout over (N, M) with 8 forward slots and 8 column-pass splits, then cnt | ps | P."""
    r4 = lambda x: (x + 3) // 4 * 4  # noqa: E731
    r64 = lambda x: (x + 63) // 64 * 64  # noqa: E731
    part = (0, 4 * 8 * n)
    stats = (part[1], part[1] + 4 * n)  # lse | row_loss | row_valid | inv_cnt
    dpart = (stats[1], stats[1] + 8 * max(n, m) * 128)
    img0 = r64(dpart[1] + 16)
    img = (img0, img0 + (n + m) * 128)
    grouped_total = img[1] + 64
    assert grouped_total == lib.rsx_nce_grouped_workspace_floats(n, m, 8, 8, 1)
    cnt0 = r4(grouped_total)
    cnt = (cnt0, cnt0 + n)
    ps = (cnt[1], cnt[1] + n)
    p0 = r4(ps[1])
    big_p = (p0, p0 + n * 128)
    return [part, stats, dpart, img, cnt, ps, big_p], big_p[1] + 16


def test_fused_workspace_regions_do_not_overlap(lib):
    for n in SIZES:
        for m in SIZES:
            regions, total = _regions(lib, n, m)
            assert lib.rsx_nce_fused_workspace_floats(n, m) == total, (n, m)
            for (b0, e0), (b1, e1) in zip(regions, regions[1:]):
                assert b0 <= e0 <= b1 <= e1 <= total, (n, m)


def test_fused_workspace_is_monotone(lib):
    tot = [[lib.rsx_nce_fused_workspace_floats(n, m) for m in SIZES] for n in SIZES]
    for a in range(len(SIZES)):
        for b in range(len(SIZES)):
            if a + 1 < len(SIZES):
                assert tot[a + 1][b] >= tot[a][b]
            if b + 1 < len(SIZES):
                assert tot[a][b + 1] >= tot[a][b]


def _view(n, m, off):
    """The plain problem as trivial groups: lab | none | beg | end | one | col_beg | col_end | colcnt."""
    rows = range(n)
    hit = [0 <= j - off < n for j in range(m)]
    return ([i + off for i in rows] + [-1] * n + list(rows) + [i + 1 for i in rows] + [1] * n
            + [j - off if h else 0 for j, h in enumerate(hit)]
            + [j - off + 1 if h else 0 for j, h in enumerate(hit)]
            + [ONE] * m)


@pytest.mark.parametrize("n,m,off", [(1, 1, 0), (5, 15, 5), (129, 129, 0)])
def test_view_arrays(lib, n, m, off):
    want = _view(n, m, off)
    assert lib.rsx_nce_view_ints(n, m) == len(want) == 5 * n + 3 * m
    buf = (ctypes.c_int * len(want))()
    assert lib.rsx_nce_view_fill_host(n, m, off, buf) == 0
    assert list(buf) == want
    # each row's exception list is its diagonal column, each column's range list that row
    for i in range(n):
        beg, end = want[2 * n + i], want[3 * n + i]
        assert want[beg:end] == [i + off]
    for j in range(m):
        cb, ce = want[5 * n + j], want[5 * n + m + j]
        assert [(want[2 * n + k], want[3 * n + k], want[4 * n + k]) for k in range(cb, ce)] == (
            [(j - off, j - off + 1, 1)] if 0 <= j - off < n else [])


def test_view_rejects_a_diagonal_outside_the_columns(lib):
    buf = (ctypes.c_int * 64)()
    assert lib.rsx_nce_view_fill_host(5, 8, 4, buf) != 0
    assert b"diag_offset" in lib.rsx_last_error()
