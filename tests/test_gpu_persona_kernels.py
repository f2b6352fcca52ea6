"""The persona passes of csrc/tx_features.hip (tx_segment_runs, tx_segment_sum_f64, tx_price_ratio) against the
oracle tests/persona_ref.py on the layouts of tests/test_gpu_tx_features_kernels.py: rows around the 256-row tile
(1, 255, 256, 257, 513, 769), one customer holding everything, a customer of 600 rows over three tiles, customers of
one row, boundaries on tile edges and an empty segment in the middle, each with three kinds of value column: runs
that cross a tile edge, one run per segment, and all-distinct values.

Bounds: runs and repeated are integers and exact; runs equals tx_segment_distinct. Each n ln n is good to a couple of
ulp and a segment sums R of them, so nlogn, and the entropy ln n - nlogn / n made from it, are within (R + 4) 2^-52
max(1, nlogn) of the oracle. A float64 sum of n values is within n 2^-53 relative of the exact sum in any order, and
bit-equal on values that are multiples of 2^-10. The device results are made once per module, twice."""
import numpy as np
import pytest
import torch

from recsys_amd import ops
from tests import persona_ref as PR

pytestmark = pytest.mark.gpu

LAYOUTS = {
    "one_row": [1],
    "all_in_one:255": [255],
    "all_in_one:256": [256],
    "tile_edge:257": [256, 1],
    "single_rows:513": [1] * 513,
    "three_tiles:769": [100, 600, 0, 69],
    "edges:769": [256, 256, 0, 257],
    "mixed:769": [3, 1, 250, 2, 0, 0, 300, 1, 1, 211],
}
KINDS = ("long_runs", "one_run", "distinct")
CASES = [f"{name}/{kind}" for name in LAYOUTS for kind in KINDS]


def _case(case):
    """(off, val sorted inside every segment, x dyadic, x float)."""
    name, kind = case.split("/")
    lens = np.asarray(LAYOUTS[name], dtype=np.int64)
    T = int(lens.sum())
    off = np.concatenate([[0], np.cumsum(lens)])
    rng = np.random.default_rng(sorted(LAYOUTS).index(name) + 31)
    val = np.zeros(T, dtype=np.int32)
    for s in range(len(lens)):
        n = int(lens[s])
        if kind == "long_runs":          # runs of about 90 rows: they cross the tile edges of the long segments
            v = np.sort(rng.integers(0, max(n // 90, 1) + 1, n))
        elif kind == "one_run":
            v = np.full(n, 7 + s)
        else:
            v = np.arange(n) * 3
        val[off[s]:off[s + 1]] = v
    return off, val, rng.integers(-512, 512, T) / 1024.0, rng.gamma(2.0, 0.7, T)


def _device(gpu, off, val, xd, xf):
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(gpu)      # noqa: E731
    T, S = len(val), len(off) - 1
    seg = ops.tx_segment_rows(up(off), T)
    runs, repeated, nlogn = ops.tx_segment_runs(seg, S, up(val))
    out = {"runs": runs, "repeated": repeated, "nlogn": nlogn, "distinct": ops.tx_segment_distinct(seg, S, up(val))}
    for key, x in (("d", xd), ("f", xf)):
        out[key + "_count"], out[key + "_sum"], out[key + "_m2"] = ops.tx_segment_sum_f64(seg, S, up(x))
    assert ops.tx_segment_sum_f64(seg, S, up(xf), m2=False)[2] is None
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def results(gpu):
    out = {}
    for case in CASES:
        data = _case(case)
        out[case] = (data, _device(gpu, *data), _device(gpu, *data))
    for g in (ops._TX_ROWS_GUARD, ops._TX_RUNS_GUARD, ops._TX_SUM_GUARD, ops._TX_DISTINCT_GUARD):
        g.check()
    return out


@pytest.mark.parametrize("case", CASES)
def test_segment_runs_equal_the_oracle(results, case):
    (off, val, _, _), got, again = results[case]
    runs, repeated, nlogn = PR.segment_runs(off, val)
    lens = np.diff(off)
    assert got["runs"].dtype == np.int32 and got["repeated"].dtype == np.int32 and got["nlogn"].dtype == np.float64
    assert got["runs"].tolist() == runs.tolist() == got["distinct"].tolist()
    assert got["repeated"].tolist() == repeated.tolist()
    bound = (runs + 4) * 2.0 ** -52 * np.maximum(1.0, nlogn)
    err = np.abs(got["nlogn"] - nlogn)
    print(f"{case}: largest |nlogn error| / bound = {(err / bound).max():.3f}")
    assert (err <= bound).all()
    n = lens.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        ent = np.where(got["runs"] > 1, np.log(n) - got["nlogn"] / n, 0.0)
    want = PR.entropy_closed_form(n, nlogn, runs)
    print(f"{case}: largest |entropy error| / bound = {(np.abs(ent - want) / bound).max():.3f}")
    assert (np.abs(ent - want) <= bound).all()
    kind = case.split("/")[1]
    if kind == "one_run":
        assert (got["runs"] == (lens > 0)).all() and (got["repeated"] == np.where(lens > 1, lens, 0)).all()
    if kind == "distinct":
        assert (got["runs"] == lens).all() and not got["repeated"].any() and not got["nlogn"].any()
    if kind == "long_runs" and lens.max() >= 600:
        s = int(lens.argmax())                                     # a run lies across a tile edge
        starts = off[s] + np.concatenate([[0], np.cumsum(PR.run_lengths(val[off[s]:off[s + 1]]))])
        assert any(a // 256 != (b - 1) // 256 for a, b in zip(starts[:-1], starts[1:]))
    for k in ("runs", "repeated", "nlogn"):
        assert not got[k][lens == 0].any(), k
        assert got[k].tobytes() == again[k].tobytes(), k


@pytest.mark.parametrize("case", [c for c in CASES if c.endswith("long_runs")])
def test_segment_sums_equal_the_oracle_within_the_summation_bound(results, case):
    (off, _, xd, xf), got, again = results[case]
    lens = np.diff(off)
    n = lens.astype(np.float64)
    cnt, tot, m2 = PR.segment_sum_f64(off, xd)
    assert got["d_count"].tolist() == cnt.tolist() == lens.tolist() and got["d_count"].dtype == np.int32
    assert (got["d_sum"] == tot).all()                             # dyadic: every partial sum is exact
    assert (np.abs(got["d_m2"] - m2) <= 1e-10 * m2 + n * (n * 2.0 ** -52) ** 2).all()
    cnt, tot, m2 = PR.segment_sum_f64(off, xf)
    err = np.abs(got["f_sum"] - tot)
    print(f"{case}: largest |sum error| / (n 2^-53 |sum|) = {(err / np.maximum(n * 2.0 ** -53 * np.abs(tot), 1e-300)).max():.3f}")
    assert (err <= n * 2.0 ** -53 * np.abs(tot)).all()
    amax = float(np.abs(xf).max())
    assert (np.abs(got["f_m2"] - m2) <= 1e-10 * m2 + n * (n * 2.0 ** -52 * amax) ** 2).all()
    for k in ("d_sum", "d_m2", "f_sum", "f_m2", "d_count"):
        assert not got[k][lens == 0].any(), k
        assert got[k].tobytes() == again[k].tobytes(), k


def test_a_flag_column_is_counted_exactly_and_a_permutation_reads_the_sorted_rows(gpu):
    rng = np.random.default_rng(4)
    T, S = 769, 9
    lab = rng.integers(0, S - 1, T).astype(np.int32)                # the last segment has no rows
    x = rng.integers(-512, 512, T) / 1024.0
    flag = (rng.random(T) < 0.3).astype(np.float64)
    up = lambda a: torch.from_numpy(a).to(gpu)      # noqa: E731
    order = torch.sort(up(lab), stable=True)
    seg, perm = order.values.contiguous(), order.indices.contiguous()
    cnt, tot, m2 = (t.cpu().numpy() for t in ops.tx_segment_sum_f64(seg, S, up(x), perm=perm))
    ops._TX_SUM_GUARD.check()
    w_cnt, w_tot, w_m2 = PR.segment_sum_f64(np.concatenate([[0], np.cumsum(np.bincount(lab, minlength=S))]), x,
                                            perm=np.argsort(lab, kind="stable"))
    assert cnt.tolist() == w_cnt.tolist() and (tot == w_tot).all() and cnt[-1] == 0 and tot[-1] == 0 and m2[-1] == 0
    assert (np.abs(m2 - w_m2) <= 1e-10 * w_m2 + 1e-24).all()
    ones = ops.tx_segment_sum_f64(seg, S, up(flag), perm=perm, m2=False)[1].cpu().numpy()
    assert ones.tolist() == np.bincount(lab, weights=flag, minlength=S).tolist()


def test_price_ratio_divides_in_float64_and_flags_an_item_or_category_out_of_range(gpu):
    rng = np.random.default_rng(6)
    T, n_items, n_cat = 513, 20, 4
    item = rng.integers(0, n_items, T).astype(np.int32)
    price = rng.gamma(2.0, 0.015, T).astype(np.float32)
    item_cat = np.sort(rng.integers(0, n_cat, n_items)).astype(np.int32)
    cat_mean = rng.gamma(2.0, 0.015, n_cat)
    up = lambda a: torch.from_numpy(a).to(gpu)      # noqa: E731
    got = ops.tx_price_ratio(up(item), up(price), up(item_cat), up(cat_mean))
    again = ops.tx_price_ratio(up(item), up(price), up(item_cat), up(cat_mean))
    ops._TX_RATIO_GUARD.check()
    want = price.astype(np.float64) / cat_mean[item_cat[item]]
    assert got.dtype == torch.float64 and (got.cpu().numpy() == want).all() and torch.equal(got, again)
    bad_item = item.copy()
    bad_item[[0, 300]] = [n_items, -1]
    got = ops.tx_price_ratio(up(bad_item), up(price), up(item_cat), up(cat_mean)).cpu().numpy()
    assert got[0] == 0.0 and got[300] == 0.0 and (np.delete(got, [0, 300]) == np.delete(want, [0, 300])).all()
    with pytest.raises(IndexError, match="tx_price_ratio"):
        ops._TX_RATIO_GUARD.check()
    bad_cat = item_cat.copy()
    bad_cat[item[5]] = n_cat
    got = ops.tx_price_ratio(up(item), up(price), up(bad_cat), up(cat_mean)).cpu().numpy()
    assert (got[item == item[5]] == 0.0).all() and (got[item != item[5]] == want[item != item[5]]).all()
    with pytest.raises(IndexError, match="tx_price_ratio"):
        ops._TX_RATIO_GUARD.check()


def test_a_decreasing_value_and_a_row_seg_out_of_order_raise_through_the_guards(gpu):
    T = 300
    seg = ops.tx_segment_rows(torch.tensor([0, 100, 300], device=gpu), T)
    val = torch.arange(T, dtype=torch.int32, device=gpu) // 4
    runs, repeated, _ = ops.tx_segment_runs(seg, 2, val)
    ops._TX_RUNS_GUARD.check()
    assert runs.tolist() == [25, 50] and repeated.tolist() == [100, 200]
    val[257] = 3                                                 # decreases inside the second segment
    ops.tx_segment_runs(seg, 2, val)
    with pytest.raises(IndexError, match="decreases"):
        ops._TX_RUNS_GUARD.check()
    val[257], val[100] = 64, 0                                   # a decrease across a boundary is none
    ops.tx_segment_runs(seg, 2, val)
    ops._TX_RUNS_GUARD.check()
    x = torch.ones(T, dtype=torch.float64, device=gpu)
    for where, value in ((299, 2), (150, 0)):                    # a segment that does not exist; a row_seg that decreases
        wrong = seg.clone()
        wrong[where] = value
        got = ops.tx_segment_runs(wrong, 2, val)
        assert int(got[1].sum()) <= T
        with pytest.raises(IndexError, match="tx_segment_runs"):
            ops._TX_RUNS_GUARD.check()
        got = ops.tx_segment_sum_f64(wrong, 2, x)
        assert int(got[0].sum()) <= T
        with pytest.raises(IndexError, match="tx_segment_sum_f64"):
            ops._TX_SUM_GUARD.check()
    perm = torch.arange(T, device=gpu)
    perm[7] = T                                                  # behind the rows: skipped
    cnt = ops.tx_segment_sum_f64(seg, 2, x, perm=perm)[0]
    assert cnt.tolist() == [99, 200]
    with pytest.raises(IndexError, match="tx_segment_sum_f64"):
        ops._TX_SUM_GUARD.check()
