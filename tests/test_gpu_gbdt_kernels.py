"""The oblivious-tree boosting kernels (csrc/gbdt.hip) one by one against the numpy oracle of
tests/gbdt_ref.py. Row counts: 1 (a single lane), 63 (a partial wave), 1000 (no multiple of the 256-thread
block), 4097 (one row past a block) and 70,001 (more than one histogram slab per feature: a slab holds at
least 8192 rows). Trees are staged through LDS 64 at a time (rsx_gbdt_tree_chunk), so the 70 trees of the
prediction test span two chunks."""
import numpy as np
import pytest
import torch

from recsys_amd import _native, ops
from tests import gbdt_ref as G

pytestmark = pytest.mark.gpu

ROWS = [1, 63, 1000, 4097, 70001]
L2 = 3.0


@pytest.fixture(scope="module")
def data():
    """Per R: the binned rows of gbdt_ref.make (column 0 rebinned to use every bin 0..255), an approximant
    with +-30 among its values, the labels and the oracle's quantised gradients. Built once, never changed."""
    out = {}
    for R in ROWS:
        num, cat, y = G.make(R, 100 + R)
        bins, is_cat, n_bins, _ = G.bin_data(num, cat)
        rng = np.random.default_rng(R)
        bins[0] = rng.integers(0, 256, R)
        bins[0, 0] = 255
        n_bins = n_bins.copy()
        n_bins[0] = 256
        F = (rng.standard_normal(R) * 4).astype(np.float32)
        F[0] = 30.0
        F[-1] = -30.0 if R > 1 else 30.0
        qg, qh = G.grad(F, y)
        out[R] = {"bins": bins, "is_cat": is_cat, "n_bins": n_bins, "F": F, "y": y, "qg": qg, "qh": qh}
    return out


def _dev(a, gpu, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a)).to(gpu)
    return t if dtype is None else t.to(dtype)


def _leaves(R, n_leaves, seed):
    """Leaf indices below n_leaves with some leaves left empty."""
    used = np.asarray([l for l in range(n_leaves) if l % 3 != 1] or [0])
    return used[np.random.default_rng(seed).integers(0, len(used), R)].astype(np.uint8)


@pytest.mark.parametrize("R", ROWS)
def test_grad_against_float64(gpu, data, R):
    d = data[R]
    qg, qh = ops.gbdt_grad(_dev(d["F"], gpu), _dev(d["y"], gpu))
    assert qg.dtype == torch.int32 and qh.dtype == torch.int32
    p = G.sigmoid64(d["F"])
    eg = np.abs(qg.cpu().numpy() / G.SCALE - (d["y"].astype(np.float64) - p)).max()
    eh = np.abs(qh.cpu().numpy() / G.SCALE - p * (1 - p)).max()
    print(f"R {R}: max |g - g64| {eg:.2e}, max |h - h64| {eh:.2e}")
    assert eg <= 2e-6 and eh <= 2e-6            # a handful of fp32 roundings on values <= 1
    assert (qh >= 0).all() and (qh <= 2 ** 28).all() and (qg.abs() <= 2 ** 30).all()


@pytest.mark.parametrize("F", [1, 12])
@pytest.mark.parametrize("n_leaves", [1, 32])
@pytest.mark.parametrize("R", ROWS)
def test_histogram_is_bit_exact(gpu, data, R, n_leaves, F):
    d = data[R]
    bins, leaf = d["bins"][:F], _leaves(R, n_leaves, R + n_leaves)
    want = G.histogram(bins, leaf, d["qg"], d["qh"], n_leaves)
    args = (_dev(bins, gpu), _dev(leaf, gpu), _dev(d["qg"], gpu, torch.int32), _dev(d["qh"], gpu, torch.int32), n_leaves)
    got = ops.gbdt_histogram(*args)
    again = ops.gbdt_histogram(*args)
    assert got.shape == (n_leaves, F, 256, 2) and got.dtype == torch.int64
    assert np.array_equal(got.cpu().numpy(), want)
    assert torch.equal(got, again)
    assert want[:, 0, 255].any()                 # bin 255 is in use
    if n_leaves == 32 and R >= 1000:
        assert not want[1].any() and want[0].any()   # an empty leaf beside a full one


def test_histogram_with_every_row_in_one_cell(gpu, data):
    d = data[70001]
    R = 70001
    bins, leaf = np.full((2, R), 7, np.uint8), np.full(R, 3, np.uint8)
    got = ops.gbdt_histogram(_dev(bins, gpu), _dev(leaf, gpu), _dev(d["qg"], gpu, torch.int32),
                             _dev(d["qh"], gpu, torch.int32), 4).cpu().numpy()
    want = np.zeros((4, 2, 256, 2), np.int64)
    want[3, :, 7] = [d["qg"].sum(), d["qh"].sum()]
    assert np.array_equal(got, want)
    assert _native.lib().rsx_gbdt_histogram_slabs(R, 2) > 1


def test_a_leaf_index_out_of_range_is_skipped_and_reported(gpu, data):
    d = data[1000]
    leaf = np.zeros(1000, np.uint8)
    leaf[17] = 4
    ops._GBDT_GUARD.check()
    got = ops.gbdt_histogram(_dev(d["bins"], gpu), _dev(leaf, gpu), _dev(d["qg"], gpu, torch.int32),
                             _dev(d["qh"], gpu, torch.int32), 4).cpu().numpy()
    keep = np.arange(1000) != 17
    assert np.array_equal(got, G.histogram(d["bins"][:, keep], leaf[keep], d["qg"][keep], d["qh"][keep], 4))
    with pytest.raises(IndexError):
        ops._GBDT_GUARD.check()


def _device_split(gpu, H, is_cat, n_bins):
    split, score = ops.gbdt_best_split(_dev(H, gpu), _dev(is_cat, gpu), _dev(n_bins, gpu), L2)
    f, b = (int(v) for v in split.cpu())
    return f, b, float(score.cpu()[0])


@pytest.mark.parametrize("n_leaves", [1, 8, 32])
@pytest.mark.parametrize("R", ROWS)
def test_best_split_scores_the_oracles_maximum(gpu, data, R, n_leaves):
    """The device's choice scores at least max (1 - 1e-12) in the oracle's fp64: the margin is fp64 rounding
    over at most 64 terms. Numeric and categorical candidates compete (7 + 5 columns)."""
    d = data[R]
    H = G.histogram(d["bins"], _leaves(R, n_leaves, 7 * R + n_leaves), d["qg"], d["qh"], n_leaves)
    S = G.scores(H, d["is_cat"], d["n_bins"], L2)
    f, b, score = _device_split(gpu, H, d["is_cat"], d["n_bins"])
    assert 0 <= f < 12 and 0 <= b < d["n_bins"][f]
    print(f"R {R}, {n_leaves} leaves: device ({f}, {b}) scores {S[f, b]!r}, the oracle's maximum is {S.max()!r}")
    assert S[f, b] >= S.max() * (1 - 1e-12)
    assert abs(score - S[f, b]) <= 1e-12 * abs(S[f, b])
    if R == 1:
        assert (f, b) == (0, 0)                  # every candidate scores the parent: the first one wins


def test_best_split_prefers_the_lower_of_two_equal_columns_and_finds_a_categorical(gpu):
    num, cat, _ = G.make(4097, 11)
    bins, is_cat, n_bins, _ = G.bin_data(num, cat)
    assert np.array_equal(bins[6], bins[0])
    F0 = np.zeros(4097, np.float32)
    for y, expect_f in (((num[:, 0] > 0.25).astype(np.float32), 0), ((cat[:, 2] == 3).astype(np.float32), 9)):
        qg, qh = G.grad(F0, y)
        H = G.histogram(bins, np.zeros(4097, np.int64), qg, qh, 1)
        S = G.scores(H, is_cat, n_bins, L2)
        f, b, _ = _device_split(gpu, H, is_cat, n_bins)
        assert (f, b) == G.best_split(S) and f == expect_f
        if expect_f == 0:
            assert S[6, b] == S[0, b] == S.max()     # an exact tie between the copies
        else:
            assert b == 3


@pytest.mark.parametrize("R", ROWS)
def test_apply_split_moves_the_leaves_exactly(gpu, data, R):
    d = data[R]
    for f, b in ((0, 100), (9, 3), (3, 250)):
        leaf = _leaves(R, 4, R + f)
        t = _dev(leaf, gpu)
        assert ops.gbdt_apply_split(_dev(d["bins"], gpu), t, torch.tensor([f, b], dtype=torch.int32, device=gpu),
                                    _dev(d["is_cat"], gpu), 4) is None
        want = 2 * leaf.astype(np.int64) + G.go_right(d["bins"], f, b, d["is_cat"])
        assert np.array_equal(t.cpu().numpy(), want)
    ops._GBDT_GUARD.check()


@pytest.mark.parametrize("split", [(0, 128), (9, 3)])
@pytest.mark.parametrize("R", ROWS)
def test_last_level_gives_leaf_sums_values_and_the_update(gpu, data, R, split):
    d = data[R]
    lr, n_leaves = 0.05, 32
    leaf = _leaves(R, n_leaves, 3 * R)
    H = G.histogram(d["bins"], leaf, d["qg"], d["qh"], n_leaves)
    t_leaf, t_F = _dev(leaf, gpu), _dev(d["F"], gpu)
    sums, values = ops.gbdt_apply_split(_dev(d["bins"], gpu), t_leaf, torch.tensor(split, dtype=torch.int32, device=gpu),
                                        _dev(d["is_cat"], gpu), n_leaves, hist=_dev(H, gpu), F=t_F, lr=lr, l2=L2)
    new_leaf = 2 * leaf.astype(np.int64) + G.go_right(d["bins"], split[0], split[1], d["is_cat"])
    want_sums, want_values = G.leaf_values(new_leaf, d["qg"], d["qh"], 2 * n_leaves, lr, L2)
    assert np.array_equal(t_leaf.cpu().numpy(), new_leaf)
    assert np.array_equal(sums.cpu().numpy(), want_sums)
    got = values.cpu().numpy()
    exact = lr * ((want_sums[:, 0] / G.SCALE) / (want_sums[:, 1] / G.SCALE + L2))
    assert np.all(np.abs(got - exact) <= 2.5e-7 * np.abs(exact))     # one fp32 rounding
    empty = np.bincount(new_leaf, minlength=2 * n_leaves) == 0
    assert empty.any() and np.all(got[empty] == 0.0) and not want_sums[empty].any()
    assert np.array_equal(t_F.cpu().numpy(), d["F"] + got[new_leaf])
    assert np.array_equal(got, want_values)
    ops._GBDT_GUARD.check()


@pytest.fixture(scope="module")
def trees(data):
    """70 random trees over the 12 columns of the shared data."""
    rng = np.random.default_rng(70)
    n_bins = data[1000]["n_bins"]
    f = rng.integers(0, 12, (70, 6))
    b = (rng.random((70, 6)) * (n_bins[f] - 1)).astype(np.int64)
    return {"splits": np.stack([f, b], axis=2), "values": (rng.standard_normal((70, 64)) * 0.1).astype(np.float32),
            "f0": np.float32(-1.3)}


@pytest.mark.parametrize("R", ROWS)
def test_predict_against_the_float64_sum(gpu, data, trees, R):
    T = 70
    assert _native.lib().rsx_gbdt_tree_chunk() == 64 < T
    d = data[R]
    model = ops.GBDTModel(_dev(trees["splits"], gpu, torch.int32), _dev(trees["values"], gpu), _dev(d["is_cat"], gpu), 6,
                          float(trees["f0"]), T)
    bins = _dev(d["bins"], gpu)
    for end in (0, 1, T):
        s64, s32, bound = G.predict(d["bins"], trees["f0"], trees["splits"], trees["values"], d["is_cat"], end)
        got = ops.gbdt_predict(bins, model, ntree_end=end).cpu().numpy()
        tol = T * 2.0 ** -23 * bound
        err = np.abs(got - s64).max()
        print(f"R {R}, {end} trees: max |device - float64| {err:.2e} (bound {tol:.2e})")
        assert err <= tol
        assert np.array_equal(got, s32)          # the fp32 additions in tree order, bit for bit
    assert np.array_equal(ops.gbdt_predict(bins, model).cpu().numpy(), got)
    head = ops.gbdt_predict(bins, model, ntree_end=33)
    ops.gbdt_predict(bins, model, ntree_begin=33, ntree_end=T, init=head, out=head)
    assert np.array_equal(head.cpu().numpy(), got)      # a running sum continues exactly
    with pytest.raises(ValueError):
        ops.gbdt_predict(bins, model, ntree_end=T + 1)


@pytest.mark.parametrize("R", ROWS)
def test_bins_against_searchsorted(gpu, R):
    rng = np.random.default_rng(R)
    x = rng.standard_normal((3, R)).astype(np.float32)
    x[1] = np.round(x[1] * 2) / 2
    x[2, ::5] = np.nan
    train = rng.standard_normal((3, 2000)).astype(np.float32)
    train[1] = np.round(train[1] * 2) / 2
    borders = [G.build_borders(train[j]) for j in range(3)]
    padded = np.full((3, 256), np.inf, np.float32)
    for j, bj in enumerate(borders):
        padded[j, :len(bj)] = bj
        x[j, :min(R, len(bj))] = bj[:R]          # values that sit exactly on a border
    n = np.asarray([len(bj) for bj in borders], np.int32)
    out = torch.full((4, R), 77, dtype=torch.uint8, device=gpu)
    got = ops.gbdt_bin(_dev(x, gpu), _dev(padded, gpu), _dev(n, gpu), out=out)
    assert got is out and (out[3] == 77).all()
    for j in range(3):
        assert np.array_equal(out[j].cpu().numpy(), G.bin_column(x[j], borders[j])), j


def test_argument_checks(gpu, data):
    d = data[63]
    bins, leaf = _dev(d["bins"], gpu), torch.zeros(63, dtype=torch.uint8, device=gpu)
    qg, qh = _dev(d["qg"], gpu, torch.int32), _dev(d["qh"], gpu, torch.int32)
    with pytest.raises(ValueError):
        ops.gbdt_histogram(bins, leaf, qg, qh, 3)
    with pytest.raises(TypeError):
        ops.gbdt_histogram(bins, leaf, qg.long(), qh, 4)
    with pytest.raises(ValueError):
        ops.gbdt_histogram(bins, leaf[:62], qg, qh, 4)
    with pytest.raises(TypeError):
        ops.gbdt_histogram(bins.int(), leaf, qg, qh, 4)
    with pytest.raises(RuntimeError):
        ops.gbdt_grad(torch.zeros(4), torch.zeros(4))
    H = torch.zeros(2, 12, 256, 2, dtype=torch.int64, device=gpu)
    with pytest.raises(ValueError):
        ops.gbdt_best_split(H, _dev(d["is_cat"], gpu), _dev(d["n_bins"], gpu), 0.0)
    with pytest.raises(ValueError):
        ops.gbdt_apply_split(bins, leaf, torch.zeros(2, dtype=torch.int32, device=gpu), _dev(d["is_cat"], gpu), 2, hist=H)
