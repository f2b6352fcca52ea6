"""CPU checks of the fused loss forward's grid (csrc/nce_common.h: fwdg_schedule, fwdg_block) through
rsx_nce_fwdg_schedule, which runs the kernels' own block-index arithmetic on the host. The library
loads without a GPU (tests/test_native_abi.py).

Rounds model: slots = 2 x CUs workgroups are co-resident; a grid of equal workgroups takes
ceil(workgroups / slots) rounds of one workgroup's length. The makespans below are in row sweeps
(one workgroup streaming all D columns = 1)."""
import ctypes
import os

import pytest

import recsys_amd  # noqa: F401
from recsys_amd import _native

ROWS = 128   # rows per row block
TILE = 32    # columns per tile


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load()


def _schedule(lib, n, d, nsplit, cus, with_blocks=False):
    sched = (ctypes.c_int64 * 7)()
    assert lib.rsx_nce_fwdg_schedule(n, d, nsplit, cus, sched, None, 0) == 0
    rb1, ns1, span1, ns2, span2, nslots, blocks = list(sched)
    out = {"rb1": rb1, "ns1": ns1, "span1": span1, "ns2": ns2, "span2": span2, "nslots": nslots, "blocks": blocks}
    if with_blocks:
        bm = (ctypes.c_int64 * (4 * max(blocks, 1)))()
        assert lib.rsx_nce_fwdg_schedule(n, d, nsplit, cus, sched, bm, blocks) == 0
        out["map"] = [tuple(bm[4 * b:4 * b + 4]) for b in range(blocks)]
    return out


def _ceil(a, b):
    return -(-a // b)


def _makespan(rb1, ns1, t, ns2, slots):
    """rounds x workgroup length of the two regions, in row sweeps"""
    return _ceil(rb1 * ns1, slots) / ns1 + _ceil(t * ns2, slots) / ns2


def test_headline_batches(lib):
    """The two batches the geometry was chosen on, at 256 CUs: whole-row leading blocks, then 173 x 8 and
    89 x 4 (8 splits of 89 row blocks model the same 1.25 sweeps; the tie goes to fewer slots)."""
    s = _schedule(lib, 153_151, 24_442, 2, 256)
    assert (s["rb1"], s["ns1"], s["ns2"], s["nslots"], s["blocks"]) == (1024, 1, 8, 8, 1024 + 173 * 8)
    assert _makespan(1024, 1, 173, 8, 512) == 2.375 and _makespan(0, 1, 1197, 2, 512) == 2.5
    s = _schedule(lib, 76_850, 16_400, 2, 256)
    assert (s["rb1"], s["ns1"], s["ns2"], s["blocks"]) == (512, 1, 4, 512 + 89 * 4)
    assert _makespan(512, 1, 89, 4, 512) == 1.25 and _makespan(0, 1, 601, 2, 512) == 1.5


@pytest.mark.parametrize("cus", [4, 8, 64, 110, 256, 304])
def test_rounds_model_choice(lib, cus):
    """nsplit 1 and 2: rb1 is the whole rounds of whole-row workgroups, ns2 the tail's best split count
    (ties to the smaller), at most 8 slots per row, and the modelled makespan never above that of
    nsplit equal splits everywhere (the geometry before the rounds model)."""
    slots = 2 * cus - (2 * cus) % 8          # whole XCD groups
    rbs_list = sorted({1, 2, 7, 8, 9, slots - 1, slots, slots + 1, slots + slots // 8, 2 * slots - 1, 2 * slots,
                       2 * slots + slots // 3, 3 * slots + 1, 5 * slots // 2} | set(range(1, 4 * slots, 37)))
    for rbs in rbs_list:
        for n in ((rbs - 1) * ROWS + 1, rbs * ROWS - 5 if rbs * ROWS > 5 else rbs * ROWS, rbs * ROWS):
            if _ceil(n, ROWS) != rbs:
                continue
            for nsplit in (1, 2):
                s = _schedule(lib, n, 1000, nsplit, cus)
                t = rbs - s["rb1"]
                assert s["ns1"] == 1 and s["rb1"] == rbs // slots * slots and 0 <= t < slots
                cands = {c: _ceil(t * c, slots) / c for c in (1, 2, 4, 8)}
                best = min(cands.values())
                assert s["ns2"] == min(c for c, v in cands.items() if v == best), (rbs, cands, s)
                assert s["nslots"] == (s["ns2"] if t else 1) and s["nslots"] <= 8
                assert s["blocks"] == s["rb1"] + t * s["ns2"]
                before = _ceil(rbs * nsplit, slots) / nsplit
                assert _makespan(s["rb1"], 1, t, s["ns2"], slots) <= before, (rbs, nsplit, s)


@pytest.mark.parametrize("cus", [8, 256])
def test_four_and_eight_slots_keep_their_geometry(lib, cus):
    """nsplit 4: four splits everywhere; nsplit 8 (the plain-family view): four splits on the row blocks
    that fill whole rounds, eight on the rest."""
    slots = 2 * cus
    for rbs in (1, 3, slots // 4, slots // 4 + 1, slots, 1197, 64):
        n = rbs * ROWS - 3
        s = _schedule(lib, n, 5000, 4, cus)
        assert (s["rb1"], s["ns1"], s["nslots"], s["blocks"]) == (rbs, 4, 4, 4 * rbs)
        s = _schedule(lib, n, 5000, 8, cus)
        rb1 = (4 * rbs // slots) * slots // 4
        assert (s["rb1"], s["ns1"], s["ns2"], s["nslots"], s["blocks"]) == (rb1, 4, 8, 8, 4 * rb1 + 8 * (rbs - rb1))


@pytest.mark.parametrize("nsplit", [1, 2, 4, 8])
def test_every_row_block_and_column_tile_is_covered_once(lib, nsplit):
    """The block map the kernels compute: every row block appears with each split of its region
    exactly once, and its splits' column ranges tile [0, D) in whole 32-column tiles without overlap
    (splits past D are empty)."""
    for cus, rbs, d in [(8, 1, 1), (8, 15, 31), (8, 16, 32), (8, 17, 33), (8, 37, 180), (8, 40, 1000), (16, 100, 257),
                        (64, 128, 4096), (64, 129, 4097), (64, 300, 100), (256, 517, 180), (256, 1197, 24_442),
                        (110, 250, 777)]:
        n = rbs * ROWS - 7
        s = _schedule(lib, n, d, nsplit, cus, with_blocks=True)
        n1 = s["rb1"] * s["ns1"]
        assert n1 % 8 == 0 or s["rb1"] == rbs  # the tail region starts on an XCD-group boundary
        seen = {}
        for b, (rb, split, j0, j1) in enumerate(s["map"]):
            lead = b < n1
            assert 0 <= rb < rbs and (rb < s["rb1"]) == lead
            ns, span = (s["ns1"], s["span1"]) if lead else (s["ns2"], s["span2"])
            assert 0 <= split < ns <= s["nslots"] <= 8
            assert span % TILE == 0 and j0 == split * span and j1 == min(j0 + span, d)
            assert (rb, split) not in seen
            seen[(rb, split)] = (j0, j1)
        assert len(seen) == s["blocks"]
        for rb in range(rbs):
            ns = s["ns1"] if rb < s["rb1"] else s["ns2"]
            ranges = sorted(seen[(rb, k)] for k in range(ns))
            ranges = [r for r in ranges if r[0] < r[1]]
            assert ranges[0][0] == 0 and ranges[-1][1] == d
            assert all(a[1] == b_[0] for a, b_ in zip(ranges, ranges[1:]))


def test_arguments_are_checked(lib):
    sched = (ctypes.c_int64 * 7)()
    assert lib.rsx_nce_fwdg_schedule(100, 100, 3, 256, sched, None, 0) == 1
    assert b"nsplit must be" in lib.rsx_last_error()
    assert lib.rsx_nce_fwdg_schedule(100, 100, 2, 256, None, None, 0) == 1
