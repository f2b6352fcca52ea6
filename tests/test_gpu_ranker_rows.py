"""The two kernels of csrc/ranker_rows.hip against tests/ranker_rows_ref.py: ops.ranker_sample_rows
(rsx_ranker_rows_sample) exactly, ops.pair_tabular (rsx_pair_tabular) against float64 and, bit for bit,
against ops.rerank_tabular on the same pairs."""
import numpy as np
import pytest
import torch

from recsys_amd import ops
from tests import ranker_rows_ref as RR

pytestmark = pytest.mark.gpu


def _csr(lists):
    off = np.zeros(len(lists) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in lists])
    flat = np.asarray([i for s in lists for i in s], np.int32)
    return off, flat


def _sample(gpu, pos_user, pos_item, lists, N, K, seed):
    off, flat = _csr(lists)
    t = lambda a: torch.from_numpy(np.asarray(a)).to(gpu)   # noqa: E731
    got = ops.ranker_sample_rows(t(np.asarray(pos_user, np.int32)), t(np.asarray(pos_item, np.int32)), t(off), t(flat),
                                 N, K, seed)
    return tuple(g.cpu().numpy() for g in got), (off, flat)


def test_sampler_equals_the_oracle_on_every_small_case(gpu):
    N, K = 5, 3
    lists = [[], [2], [0, 1, 3, 4], [0], [N - 1], [1, 3]]        # D = 0, 1, 4 (one item left), {0}, {N - 1}, 2
    pos_user = [0, 1, 2, 2, 3, 4, 2, 5, 5, 5, 1, 0, 3, 4]
    pos_item = [3, 2, 0, 0, 0, 4, 4, 1, 3, 1, 2, 0, 0, 4]        # repeated positives: (2, 0), (5, 1), (1, 2)
    ops._RANKER_ROWS_GUARD.check()
    (ru, ri, y), (off, flat) = _sample(gpu, pos_user, pos_item, lists, N, K, 42)
    ops._RANKER_ROWS_GUARD.check()
    wu, wi, wy = RR.sample(pos_user, pos_item, off, flat, N, K, 42)
    assert ru.dtype == ri.dtype == np.int32 and y.dtype == np.float32
    assert np.array_equal(ru, wu) and np.array_equal(ri, wi) and np.array_equal(y, wy)
    rows = ri.reshape(-1, K + 1)
    for p, u in enumerate(pos_user):
        assert not set(rows[p, 1:].tolist()) & set(lists[u]), p           # a negative is never a bought item
        if u == 2:
            assert rows[p, 1:].tolist() == [2, 2, 2]                      # the one item left
    assert len({tuple(r[1:]) for r, u in zip(rows, pos_user) if u == 0}) > 1


def test_sampler_equals_the_oracle_with_a_long_bought_list(gpu):
    N, K, Pv = 70001, 5, 300
    rng = np.random.default_rng(3)
    lists = [np.sort(rng.permutation(N)[:n]).tolist() for n in (1000, 0, 7, 1, 250)]
    lists[3] = [N - 1]
    pos_user = rng.integers(0, 5, Pv)
    pos_user[:60] = 0
    pos_item = rng.integers(0, N, Pv)
    (ru, ri, y), (off, flat) = _sample(gpu, pos_user, pos_item, lists, N, K, 2 ** 63 + 11)
    ops._RANKER_ROWS_GUARD.check()
    wu, wi, wy = RR.sample(pos_user, pos_item, off, flat, N, K, 2 ** 63 + 11)
    assert np.array_equal(ru, wu) and np.array_equal(ri, wi) and np.array_equal(y, wy)
    neg = ri.reshape(Pv, K + 1)[:60, 1:].reshape(-1)
    assert not np.isin(neg, lists[0]).any() and neg.min() >= 0 and neg.max() < N


def test_no_negatives_two_calls_and_another_seed(gpu):
    N = 50
    lists = [[1, 5, 7], [0], []]
    pos_user, pos_item = [0, 0, 1, 2, 2, 0], [1, 5, 0, 9, 9, 7]
    (ru, ri, y), _ = _sample(gpu, pos_user, pos_item, lists, N, 0, 1)
    assert ru.tolist() == pos_user and ri.tolist() == pos_item and y.tolist() == [1.0] * 6      # K = 0: positives only
    a, _ = _sample(gpu, pos_user, pos_item, lists, N, 8, 1)
    b, _ = _sample(gpu, pos_user, pos_item, lists, N, 8, 1)
    c, _ = _sample(gpu, pos_user, pos_item, lists, N, 8, 2)
    ops._RANKER_ROWS_GUARD.check()
    assert all(np.array_equal(x, z) for x, z in zip(a, b))                                     # the same bits every run
    assert np.array_equal(a[0], c[0]) and np.array_equal(a[2], c[2]) and not np.array_equal(a[1], c[1])


def test_a_customer_who_bought_everything_and_an_item_out_of_range_are_reported(gpu):
    ops._RANKER_ROWS_GUARD.check()
    (ru, ri, y), _ = _sample(gpu, [0, 1], [1, 2], [[0, 1, 2], [0]], 3, 2, 5)       # D = N: the call returns
    with pytest.raises(IndexError):
        ops._RANKER_ROWS_GUARD.check()
    assert ri[:3].tolist() == [1, 0, 0] and set(ri[4:].tolist()) <= {1, 2} and y.tolist() == [1, 0, 0, 1, 0, 0]
    (ru, ri, y), _ = _sample(gpu, [0, 1], [1, 3], [[0], [0]], 3, 1, 5)             # pos_item 3 >= N
    with pytest.raises(IndexError):
        ops._RANKER_ROWS_GUARD.check()
    assert ri[2] == 0
    (ru, ri, y), _ = _sample(gpu, [0, 2], [1, 1], [[0], [0]], 3, 1, 5)             # pos_user 2 >= C
    with pytest.raises(IndexError):
        ops._RANKER_ROWS_GUARD.check()
    _sample(gpu, [0, 1], [1, 2], [[0], [0]], 3, 1, 5)
    ops._RANKER_ROWS_GUARD.check()                                                 # a good call raises nothing
    z = torch.zeros(2, dtype=torch.int32, device=gpu)
    off = torch.zeros(3, dtype=torch.int64, device=gpu)
    with pytest.raises(ValueError):
        ops.ranker_sample_rows(z, z, off, z[:0], 3, -1, 0)
    with pytest.raises(TypeError):
        ops.ranker_sample_rows(z.long(), z, off, z[:0], 3, 1, 0)


C, N, D = 5, 300, 128


@pytest.fixture(scope="module")
def tables():
    rng = np.random.default_rng(0)
    norm = lambda x: x / np.linalg.norm(x, axis=1, keepdims=True)   # noqa: E731
    U, V = norm(rng.standard_normal((C, D))).astype(np.float32), norm(rng.standard_normal((N, D))).astype(np.float32)
    price = (rng.random(N) * 90 + 5).astype(np.float32)
    avg = np.asarray([30.0, 0.0, 55.5, -3.0, 80.0], np.float32)
    return U, V, price, avg


@pytest.mark.parametrize("R", [1, 65])
def test_pair_tabular_against_float64_and_rerank_tabular(gpu, tables, R):
    U, V, price, avg = tables
    rng = np.random.default_rng(R)
    row_user, row_item = rng.integers(0, C, R).astype(np.int32), rng.integers(0, N, R).astype(np.int32)
    row_user[0] = 1 if R == 1 else row_user[0]
    if R > 1:
        row_user[:5] = np.arange(5)                                # every user, avg <= 0 among them
    score = rng.standard_normal(R).astype(np.float32)
    t = lambda a: torch.from_numpy(a).to(gpu)   # noqa: E731
    dU, dV, dp, da = t(U), t(V), t(price), t(avg)
    ops._PAIR_GUARD.check()
    given = ops.pair_tabular(t(row_user), t(row_item), t(score), dU, dV, dp, da)
    dotted = ops.pair_tabular(t(row_user), t(row_item), None, dU, dV, dp, da)
    ops._PAIR_GUARD.check()
    assert given.shape == dotted.shape == (7, R) and given.dtype == torch.float32
    want, scale = RR.columns(row_user, row_item, score, U, V, price, avg)
    want_dot, _ = RR.columns(row_user, row_item, None, U, V, price, avg)
    tol = 128 * 2.0 ** -23 * scale
    g, dt = given.cpu().numpy(), dotted.cpu().numpy()
    errs = [np.abs(g[j] - want[j]).max() for j in (1, 2, 3)] + [np.abs(dt[0] - want_dot[0]).max()]
    print(f"R {R}: max error of mean / max / std / dot: " + " / ".join(f"{e:.2e}" for e in errs) + f" (bound {tol:.2e})")
    assert max(errs) <= tol
    assert np.array_equal(g[0], score) and np.array_equal(g[1:], dt[1:])
    assert np.array_equal(g[4], price[row_item]) and np.array_equal(g[5], avg[row_user])
    assert np.all(np.abs(g[6] - want[6]) <= 2.0 ** -22 * np.abs(want[6]))          # two fp32 roundings
    assert np.all(g[6][avg[row_user] <= 0] == 0.0) and (avg[row_user] <= 0).any()  # avg <= 0 gives ratio 0
    # the serving kernel on the same pairs, one query per row: columns 1..6 bit for bit, the score copied
    serve, ids = ops.rerank_tabular(t(row_item.astype(np.int64)).view(R, 1), t(score).view(R, 1),
                                    dU.index_select(0, t(row_user).long()), dV, dp, da.index_select(0, t(row_user).long()))
    ops._RERANK_GUARD.check()
    assert torch.equal(serve, given)


def test_pair_tabular_labels_and_ids_out_of_range(gpu, tables):
    U, V, price, avg = tables
    t = lambda a: torch.from_numpy(np.asarray(a)).to(gpu)   # noqa: E731
    truth = [[3, 9, 200], [], [0], [299], [5, 6, 7, 8]]
    off, flat = _csr(truth)
    row_user = np.asarray([0, 0, 0, 1, 2, 2, 3, 3, 4, 4, 4, 0], np.int32)
    row_item = np.asarray([9, 10, 200, 3, 0, 1, 299, 298, 4, 5, 8, 3], np.int32)
    ops._PAIR_GUARD.check()
    feats, y = ops.pair_tabular(t(row_user), t(row_item), None, t(U), t(V), t(price), t(avg), t(off), t(flat))
    ops._PAIR_GUARD.check()
    assert y.cpu().tolist() == [1, 0, 1, 0, 1, 0, 1, 0, 0, 1, 1, 1]               # a hit, a miss, an empty truth set
    plain = ops.pair_tabular(t(row_user), t(row_item), None, t(U), t(V), t(price), t(avg))
    assert torch.equal(plain, feats)
    bad_user, bad_item = row_user.copy(), row_item.copy()
    bad_user[1], bad_item[4], bad_item[7] = C, N, -1
    feats, y = ops.pair_tabular(t(bad_user), t(bad_item), None, t(U), t(V), t(price), t(avg), t(off), t(flat))
    with pytest.raises(IndexError):
        ops._PAIR_GUARD.check()
    f = feats.cpu().numpy()
    assert f[5, 1] == avg[0] and f[4, 4] == price[0] and f[4, 7] == price[0]      # the id used is 0
    keep = np.ones(len(row_user), bool)
    keep[[1, 4, 7]] = False
    assert np.array_equal(f[:, keep], plain.cpu().numpy()[:, keep])
    with pytest.raises(TypeError):
        ops.pair_tabular(t(row_user).long(), t(row_item), None, t(U), t(V), t(price), t(avg))
    with pytest.raises(ValueError):
        ops.pair_tabular(t(row_user), t(row_item)[:3], None, t(U), t(V), t(price), t(avg))
    with pytest.raises(ValueError):
        ops.pair_tabular(t(row_user), t(row_item), None, t(U), t(V), t(price), t(avg)[:2])
