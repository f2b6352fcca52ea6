"""The QuerySoftMax oracle (tests/gbdt_rank_ref.py) against independent restatements, on the CPU: a plain
per-group float64 softmax, central differences of its own loss, and a permutation of the rows."""
import numpy as np

from tests import gbdt_rank_ref as Q
from tests import gbdt_ref as G

R = 2048


def _rows(seed=3):
    rng = np.random.default_rng(seed)
    gid = Q.layout(R, 11)
    F = (2.0 * rng.standard_normal(R)).astype(np.float32)
    F[:4] = (30.0, -30.0, 30.0, -30.0)
    y = (rng.random(R) < 0.3).astype(np.float32)
    return F, y, gid


def test_layout_follows_its_sizes():
    gid = Q.layout(4096, 7)
    ids, counts = np.unique(gid, return_counts=True)
    assert list(counts[:len(Q.SIZES)]) == list(Q.SIZES) and set(counts[len(Q.SIZES):-1]) == {6}
    assert np.array_equal(ids, 3 * np.arange(len(ids)) + 5) and counts.sum() == 4096
    assert not np.all(np.diff(gid) >= 0)          # scattered


def test_gradients_match_a_plain_float64_softmax():
    F, y, gid = _rows()
    g, h = Q.grad_float(F, y, gid)
    g64, h64 = Q.grad_plain64(F, y, gid)
    print(f"max |g - g64| {np.abs(g - g64).max():.3e}, max |h - h64| {np.abs(h - h64).max():.3e}")
    assert np.abs(g - g64).max() <= 2e-6 and np.abs(h - h64).max() <= 2e-6
    qg, qh = Q.grad(F, y, gid)
    assert np.abs(qg).max() <= 2 ** 30 and qh.min() >= 0 and qh.max() <= 2 ** 28
    assert np.abs(qg / G.SCALE - g64).max() <= 2e-6 and np.abs(qh / G.SCALE - h64).max() <= 2e-6
    dead = np.isin(gid, [q for q in np.unique(gid) if (y[gid == q] == 1).sum() == 0])
    assert dead.any() and not qg[dead].any() and not qh[dead].any()


def test_gradient_is_the_central_difference_of_the_loss():
    """g = -dL/da of the summed loss. With the step 2^-7 (the two sides differ by float32 roundings, below 2^-21:
    times L'' <= 1/4 that is 1e-7) the third derivative of a log-softmax, below 0.1, leaves a truncation error
    below (2^-7)^2 / 6 * 0.1 < 2e-6, and the loss's own 2^-33 quantisation of E adds 2^-33 / 2^-7 < 1e-7 per
    term: 1e-5 covers them."""
    F, y, gid = _rows()
    g, _ = Q.grad_float(F, y, gid)
    step = np.float32(2.0 ** -7)
    rows = np.random.default_rng(0).choice(np.flatnonzero(np.abs(F) < 8), 48, replace=False)
    for i in rows:
        up, down = F.copy(), F.copy()
        up[i] += step
        down[i] -= step
        width = float(up[i]) - float(down[i])       # the float32 values' own distance: 2^-6 up to two roundings
        assert abs(width - 2.0 * float(step)) <= 2.0 ** -20
        slope = (Q.loss_sum(up, y, gid)[0] - Q.loss_sum(down, y, gid)[0]) / width
        assert abs(-slope - float(g[i])) <= 1e-5, (i, slope, g[i])


def test_a_permutation_of_the_rows_permutes_the_gradients_bit_for_bit():
    F, y, gid = _rows()
    qg, qh = Q.grad(F, y, gid)
    perm = np.random.default_rng(1).permutation(R)
    pg, ph = Q.grad(F[perm], y[perm], gid[perm])
    assert np.array_equal(pg, qg[perm]) and np.array_equal(ph, qh[perm])
    assert Q.loss_sum(F[perm], y[perm], gid[perm])[1] == Q.loss_sum(F, y, gid)[1]


def test_equal_scores_give_uniform_probabilities_and_a_log_n_loss():
    gid = np.repeat([4, 9], [5, 3])
    y = np.asarray([1, 0, 0, 0, 0, 0, 0, 0], np.float32)
    F = np.full(8, 1.25, np.float32)
    g, h = Q.grad_float(F, y, gid)
    assert np.allclose(g[:5], [0.8, -0.2, -0.2, -0.2, -0.2], atol=1e-7) and np.allclose(h[:5], 0.16, atol=1e-7)
    assert not g[5:].any() and not h[5:].any()
    total, live = Q.loss_sum(F, y, gid)
    assert live == 1 and abs(total - np.log(5.0)) < 1e-9       # Z = 5 2^32 exactly
