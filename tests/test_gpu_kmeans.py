"""The k-means kernels (csrc/kmeans.hip) against the numpy oracle of tests/persona_ref.py, which runs the same
algorithm on the same integers in the same floating-point order: given the starting centres, the labels, the centres
and the iteration count are equal bit for bit. The inertia is a float64 sum of C squared distances in another order:
within C 2^-52 relative. Shapes: C in {1, 255, 256, 257, 769} rows around the 256-row tile, (K, d) in {(1, 1), (2, 7),
(20, 7), (7, 32), (256, 16)}: the smallest, the personas' width, the widest row, and the largest K d (the 64 KB form
of the assignment kernel; K d <= 512 takes the small one). max_workgroups = 2 at 769 rows makes a workgroup stride
over two tiles. The standardised columns are checked against the oracle's exact sums within C 2^-52 relative of
the column's largest magnitude. The oracle's fits are made once per module."""
import numpy as np
import pytest
import torch

from recsys_amd import ops
from tests import persona_ref as PR

pytestmark = pytest.mark.gpu

SHAPES = [(C, K, d) for C in (1, 255, 256, 257, 769) for K, d in ((1, 1), (2, 7), (20, 7), (7, 32), (256, 16)) if K <= C]


def _blob_case(C, K, d, seed=0):
    X, _ = PR.blobs(C, K, d, seed)
    Z = PR.standardize(X)[0]
    bits = PR.frac_bits(Z)
    q = PR.quantize(Z, bits)
    x = (q.astype(np.float64) * 2.0 ** -bits).T
    rows = np.random.default_rng(seed + 1).permutation(C)[:K]
    return q, bits, x[rows]


def _fit(gpu, q, bits, init, tol_abs=0.0, max_iter=300, max_workgroups=None, poll=ops.KMEANS_POLL):
    fit = ops.kmeans_fit(torch.from_numpy(np.ascontiguousarray(q, dtype=np.int32)).to(gpu), bits, torch.from_numpy(np.ascontiguousarray(init)).to(gpu),
                         tol_abs, max_iter, max_workgroups, poll)
    return (fit.centres.cpu().numpy(), fit.labels.cpu().numpy(), fit.dmin.cpu().numpy(), fit.n_iter,
            fit.counts.cpu().numpy(), float(fit.inertia))


def _same(got, want, C):
    centres, labels, dmin, n_iter, counts = want
    assert got[3] == n_iter
    assert got[1].dtype == np.int32 and got[1].tolist() == labels.tolist()
    assert got[0].tobytes() == centres.tobytes()
    assert got[2].tobytes() == dmin.tobytes()
    assert got[4].tolist() == counts.tolist()
    inertia = float(np.sum(dmin))
    assert abs(got[5] - inertia) <= C * 2.0 ** -52 * inertia


@pytest.mark.parametrize("C,K,d", SHAPES)
def test_a_fit_from_given_centres_equals_the_oracle_bit_for_bit(gpu, C, K, d):
    q, bits, init = _blob_case(C, K, d)
    tol_abs = 1e-4 * float(np.var(q.astype(np.float64) * 2.0 ** -bits, axis=1).mean())
    for tol in (tol_abs, 0.0):
        want = PR.lloyd(q, bits, init, tol)
        got = _fit(gpu, q, bits, init, tol)
        _same(got, want, C)
        again = _fit(gpu, q, bits, init, tol, max_workgroups=2, poll=3)        # the stride loop; another polling interval
        assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, again))
    print(f"C {C} K {K} d {d}: n_iter {want[3]}, frac_bits {bits}")


@pytest.fixture(scope="module")
def gaussian():
    """One Gaussian, K = 8: nothing to separate, the fit runs tens of iterations."""
    rng = np.random.default_rng(12)
    Z = PR.standardize(rng.standard_normal((7, 769)))[0]
    bits = PR.frac_bits(Z)
    q = PR.quantize(Z, bits)
    init = (q.astype(np.float64) * 2.0 ** -bits).T[rng.permutation(769)[:8]]
    return q, bits, init, PR.lloyd(q, bits, init, 0.0), PR.lloyd(q, bits, init, 0.0, max_iter=1)


def test_a_long_fit_ends_on_unchanged_labels_with_tol_0_and_is_the_same_bits_with_the_rows_permuted(gpu, gaussian):
    q, bits, init, want, _ = gaussian
    assert 10 <= want[3] < 300
    got = _fit(gpu, q, bits, init, 0.0)
    _same(got, want, 769)
    assert np.array_equal(PR.assign(q, bits, want[0])[0], want[1])             # ended on changed == 0: a fixed point
    perm = np.random.default_rng(2).permutation(769)
    moved = _fit(gpu, q[:, perm], bits, init, 0.0, max_workgroups=2)
    assert moved[0].tobytes() == got[0].tobytes() and moved[3] == got[3]
    assert moved[1].tolist() == got[1][perm].tolist() and moved[2].tobytes() == got[2][perm].tobytes()
    again = _fit(gpu, q, bits, init, 0.0)
    assert all(np.asarray(a).tobytes() == np.asarray(b).tobytes() for a, b in zip(got, again))
    # a tolerance the shift passes half way: the same stop as the oracle's
    half = PR.lloyd(q, bits, init, 1e-3)
    assert half[3] < want[3]
    _same(_fit(gpu, q, bits, init, 1e-3), half, 769)


def test_max_iter_1_stops_unconverged(gpu, gaussian):
    q, bits, init, full, want = gaussian
    assert want[3] == 1 and want[0].tobytes() != full[0].tobytes()
    _same(_fit(gpu, q, bits, init, 0.0, max_iter=1), want, 769)
    nine = PR.lloyd(q, bits, init, 0.0, max_iter=9)                              # not a multiple of the polling interval
    assert nine[3] == 9
    _same(_fit(gpu, q, bits, init, 0.0, max_iter=9), nine, 769)


def test_a_point_midway_between_two_centres_goes_to_the_lower_index_and_an_empty_cluster_keeps_its_centre(gpu):
    bits = 4
    q = np.asarray([[0, 16, 32, 48, 64, 64], [0, 0, 0, 0, 0, 16]], dtype=np.int64)      # x = 0, 1, 2, 3, 4, 4
    centres = np.asarray([[3.0, 0.0], [1.0, 0.0], [3.0, 0.0]])                 # x = 2 is midway between 0 / 2 and 1
    labels, dmin, _ = ops.kmeans_assign(torch.from_numpy(q.astype(np.int32)).to(gpu), bits, torch.from_numpy(centres).to(gpu))
    assert labels.tolist() == [1, 1, 0, 0, 0, 0] and dmin.tolist() == [1.0, 0.0, 1.0, 0.0, 1.0, 2.0]
    assert PR.assign(q, bits, centres)[0].tolist() == labels.tolist()
    # a duplicate seed: the lower index takes the rows, the other stays empty and keeps its centre
    q = np.asarray([[0, 0, 0, 64, 64, 80], [0, 0, 0, 0, 16, 0]], dtype=np.int64)        # (0, 0) three times; (4, 0), (4, 1), (5, 0)
    centres = np.asarray([[0.0, 0.0], [4.0, 0.0], [0.0, 0.0]])
    want = PR.lloyd(q, bits, centres, 0.0)
    got = _fit(gpu, q, bits, centres, 0.0)
    _same(got, want, 6)
    assert got[1].tolist() == [0, 0, 0, 1, 1, 1] and got[4].tolist() == [3, 3, 0]
    assert got[0][2].tolist() == [0.0, 0.0] and got[0][1].tolist() == [13.0 / 3.0, 1.0 / 3.0]


def test_quantize_rounds_to_even_and_a_value_too_large_for_frac_bits_raises(gpu):
    X = torch.tensor([[0.5, 1.5, 2.5, -0.5, -1.5, 1023.25]], dtype=torch.float64, device=gpu)
    q, bits = ops.kmeans_quantize(X, 0)
    assert q.tolist() == [[0, 2, 2, 0, -2, 1023]] and q.dtype == torch.int32
    q, bits = ops.kmeans_quantize(X)
    assert bits == 20 and q.tolist() == PR.quantize(X.cpu().numpy(), 20).tolist()
    assert ops.kmeans_frac_bits(torch.tensor([[1024.0]], device=gpu, dtype=torch.float64)) == 20
    assert ops.kmeans_frac_bits(torch.tensor([[1025.0]], device=gpu, dtype=torch.float64)) == 19
    assert ops.kmeans_frac_bits(torch.zeros(1, 3, device=gpu, dtype=torch.float64)) == 20
    assert PR.frac_bits(np.asarray([[1025.0]])) == 19
    with pytest.raises(ValueError, match="does not fit"):
        ops.kmeans_quantize(X, 22)                                             # 1023.25 * 2^22 >= 2^31
    with pytest.raises(ValueError, match="NaN"):
        ops.kmeans_quantize(torch.tensor([[0.0, float("nan")]], dtype=torch.float64, device=gpu), 20)
    with pytest.raises(ValueError, match="NaN"):
        ops.kmeans_quantize(torch.tensor([[0.0, float("nan")]], dtype=torch.float64, device=gpu))
    with pytest.raises(ValueError, match="d <= 32"):
        ops.kmeans_seed(torch.zeros(33, 4, dtype=torch.int32, device=gpu), 20, 2, 0)
    with pytest.raises(ValueError, match="K d <= 4096"):
        ops.kmeans_seed(torch.zeros(32, 300, dtype=torch.int32, device=gpu), 20, 129, 0)


@pytest.mark.parametrize("C,d", [(1, 1), (257, 7), (769, 3), (5000, 2)])
def test_standardize_columns_equals_the_oracle(gpu, C, d):
    rng = np.random.default_rng(C)
    X = rng.gamma(2.0, 3.0, (d, C)) - 4.0
    X[d - 1] = 0.1                                                             # a constant column
    Z, mean, scale, var = (t.cpu().numpy() for t in ops.standardize_columns(torch.from_numpy(X).to(gpu)))
    again = ops.standardize_columns(torch.from_numpy(X).to(gpu))
    wz, wm, ws, wv = PR.standardize(X)
    # mean: a sum of C values within C 2^-53 sum |x|; var: the same of C squares up to (2 big)^2; scale = sqrt(var) and
    # z = (x - mean) / scale carry these over, times big / scale >= 1 for every further division
    big = np.abs(X).max(axis=1)
    u = C * 2.0 ** -52
    assert (np.abs(mean - wm) <= u * big).all()
    assert (np.abs(var - wv) <= 4 * u * big ** 2).all()
    assert scale[d - 1] == 1.0 and ws[d - 1] == 1.0 and np.abs(Z[d - 1]).max() <= u * 0.1
    if C > 1:
        ratio = big[:-1] / ws[:-1]
        assert (np.abs(scale[:-1] - ws[:-1]) <= 4 * u * big[:-1] * ratio).all()
        assert (np.abs(Z[:-1] - wz[:-1]).max(axis=1) <= 10 * u * ratio ** 3).all()
    else:
        assert scale.tolist() == [1.0] and Z.tolist() == [[0.0]]
    assert all(torch.equal(a, b) for a, b in zip(ops.standardize_columns(torch.from_numpy(X).to(gpu)), again))
    moments = ops.standardize_columns(torch.from_numpy(X).to(gpu), out=False)
    assert moments[0] is None and torch.equal(moments[3], again[3])


# ---- seeding ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C,K,d,max_workgroups", [(1, 1, 1, None), (255, 2, 7, None), (769, 20, 7, 2), (769, 7, 32, None),
                                                  (257, 256, 16, None)])
def test_every_seed_has_a_key_within_2_pow_minus_48_of_the_rounds_largest(gpu, C, K, d, max_workgroups):
    q, bits, _ = _blob_case(C, K, d, seed=3)
    qd = torch.from_numpy(q.astype(np.int32)).to(gpu)
    seed = 1234 + C
    seeds, centres = ops.kmeans_seed(qd, bits, K, seed, max_workgroups)
    again = ops.kmeans_seed(qd, bits, K, seed)                                 # another grid: the same rows
    assert torch.equal(seeds, again[0]) and torch.equal(centres, again[1]) and seeds.dtype == torch.int32
    rows = seeds.cpu().numpy()
    assert rows[0] == int(PR.DR.hash_u32(seed, [0])[0]) % C
    assert centres.cpu().numpy().tobytes() == (q.astype(np.float64) * 2.0 ** -bits).T[rows].tobytes()
    assert len(set(rows.tolist())) == K                                        # the data have >= K distinct points
    dmin = None
    for r in range(1, K):                                                      # every round, along the device's own choices
        dmin, key = PR.seed_round(q, bits, seed, r, rows[r - 1], dmin)
        assert key[rows[r]] >= (1.0 - 2.0 ** -48) * key.max(), r
        assert dmin[rows[r]] > 0.0 or not dmin.any(), r


def test_seeding_never_draws_a_covered_point_while_another_is_left(gpu):
    """Four distinct points, each 64 times over, K = 6: the first four seeds are the four points, then dmin is 0
    everywhere and the lowest row wins."""
    base = np.asarray([[0, 5, 9, 14]], dtype=np.int64) << 16
    q = np.repeat(base, 64, axis=1)[:, np.random.default_rng(0).permutation(256)]
    for seed in range(5):
        rows = ops.kmeans_seed(torch.from_numpy(q.astype(np.int32)).to(gpu), 16, 6, seed)[0].cpu().numpy()
        assert sorted(q[0, rows[:4]].tolist()) == base[0].tolist()
        assert rows[4:].tolist() == [0, 0] and PR.seeds(q, 16, 6, seed)[4:].tolist() == [0, 0]
