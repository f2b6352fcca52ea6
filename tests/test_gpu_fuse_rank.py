"""ops.fuse_rank (csrc/ensemble.hip, fuse_rank_k) against tests/ensemble_ref.py.

(a) the raw scores against the float64 dot product, within the bound of a D-term fp32 sum;
(b) everything downstream of the scores, exactly, when the reference is fed the device's own scores:
    both modes, pool sizes 1 / 3 / 128 / 2000 / 2048 (one entry, an odd pool, one that fills a sort's
    power of two, the evaluators' default, the limit), 1 and 11 alphas, pools with full / no / partial
    overlap, truths of 0 / 1 / 300 items partly absent from the pool, a constant list, the cut quirk;
(c) exact-grid inputs, where every dot product is exact in fp32 in any order: scores, hits and lists
    equal the reference end to end."""
import functools

import numpy as np
import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import ops
from recsys_amd.tower_code import mined_inference as MI
from tests import ensemble_ref as REF

pytestmark = pytest.mark.gpu

NI, DA, DB, Q = 6000, 64, 128, 6
TRUTH_LENS = [0, 1, 300, 1, 7, 300]
POOL_SIZES = [1, 3, 128, 2000, 2048]
ALPHAS = {1: [0.3], 11: MI.alpha_grid(0.1)}


@functools.lru_cache(maxsize=None)
def _vectors(kind):
    rng = np.random.default_rng(7 if kind == "gaussian" else 8)

    def make(n, d):
        if kind == "gaussian":
            x = rng.standard_normal((n, d))
            return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)
        return (rng.integers(-16, 17, size=(n, d)) / 16.0).astype(np.float32)   # multiples of 2^-4 in [-1, 1]

    out = make(Q, DA), make(NI, DA), make(Q, DB), make(NI, DB)
    for t in out:
        t.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _pool(C, overlap):
    """cand [Q, C] int32 = cat([pool_a, pool_b]), each pool of distinct ids; pool_b repeats all / none /
    half of pool_a's ids (as far as the sizes allow), in another order."""
    rng = np.random.default_rng(100 + C + {"full": 0, "none": 1, "partial": 2}[overlap])
    na, nb = C - C // 2, C // 2
    cand = np.empty((Q, C), dtype=np.int32)
    for q in range(Q):
        ids = rng.permutation(NI)
        a = ids[:na]
        shared = {"full": nb, "none": 0, "partial": nb // 2}[overlap]
        b = np.concatenate([rng.permutation(a)[:shared], ids[na:na + nb - shared]])
        cand[q] = np.concatenate([a, rng.permutation(b)])
    cand.setflags(write=False)
    return cand


def _truth(cand, seed=0):
    """One set per user, of TRUTH_LENS items: about half of them pool entries, the rest absent from the
    pool (user 3's single item is absent, user 1's is a pool entry)."""
    rng = np.random.default_rng(200 + seed)
    out = []
    for q, n in enumerate(TRUTH_LENS):
        n_in = 0 if q == 3 else min(n - n // 2, cand.shape[1])
        inside = rng.choice(cand[q], size=n_in, replace=False) if n_in else np.zeros(0, int)
        outside = np.setdiff1d(np.arange(NI), cand[q])[: n - len(set(inside.tolist()))]
        out.append(set(inside.tolist()) | set(outside.tolist()))
    return out


def _ks(C, cut):
    return sorted({min(k, cut) for k in (1, 5, 20, 100, 500)})


def _run(gpu, vecs, cand, truth, alphas, mode, cut, ks, k_rrf=200.0):
    ua, Ia, ub, Ib = (torch.tensor(t).to(gpu) for t in vecs)
    off, tr = MI.truth_csr({q: t for q, t in enumerate(truth)}, list(range(len(truth))), NI)
    out = ops.fuse_rank(ua, Ia, ub, Ib, torch.tensor(cand).to(gpu), alphas, ks, torch.tensor(off).to(gpu),
                        torch.tensor(tr).to(gpu), mode=mode, k_rrf=k_rrf, cut=cut, return_lists=True,
                        return_scores=True)
    assert out.flag.item() == 0
    return out.hits.cpu().numpy(), out.lists.cpu().numpy(), out.sa.cpu().numpy(), out.sb.cpu().numpy()


def _downstream(gpu, vecs, cand, truth, alphas, mode, cut):
    """The kernel's hits and lists equal the reference fed the kernel's own scores."""
    ks = _ks(cand.shape[1], cut)
    hits, lists, sa, sb = _run(gpu, vecs, cand, truth, alphas, mode, cut, ks)
    wa, wb = REF.fusion_weights(alphas)
    rh, rl = REF.fuse_rank(sa, sb, cand, wa, wb, mode, 200.0, cut, ks, truth)
    assert np.array_equal(lists, rl), f"lists differ (first at {np.argwhere(lists != rl)[:3].tolist()})"
    assert np.array_equal(hits, rh)
    return hits, lists, sa, sb


def test_scores_lie_within_the_fp32_sum_bound_of_float64(gpu):
    """|s - s64| <= (D + 2) u sum |u_i| |v_i|, u = 2^-24: each term of a D-term fp32 dot product passes
    through at most D roundings (its product, unless an FMA absorbs it, and at most D - 1 additions, in
    any order), so the error is at most gamma_D = D u / (1 - D u) of that sum, which is below (D + 1) u
    for D <= 128; the float64 side's own gamma_D (u = 2^-53) is far below the one u left over."""
    vecs = _vectors("gaussian")
    cand = _pool(2000, "partial")
    _, _, sa, sb = _run(gpu, vecs, cand, _truth(cand), [0.5], "minmax", 520, [5])
    ua, Ia, ub, Ib = vecs
    for s, u, I, D in ((sa, ua, Ia, DA), (sb, ub, Ib, DB)):
        for q in range(Q):
            want, mag = REF.dot64(u[q], I[cand[q]])
            err = np.abs(s[q].astype(np.float64) - want)
            assert np.all(err <= (D + 2) * 2.0 ** -24 * mag), (D, q, float((err / mag).max()))


@pytest.mark.parametrize("overlap", ["full", "none", "partial"])
@pytest.mark.parametrize("A", [1, 11])
@pytest.mark.parametrize("C", POOL_SIZES)
@pytest.mark.parametrize("mode", ["minmax", "rrf"])
def test_downstream_of_the_device_scores_is_exact(gpu, mode, C, A, overlap):
    cand = _pool(C, overlap)
    _downstream(gpu, _vectors("gaussian"), cand, _truth(cand), ALPHAS[A], mode, min(C, 520))


@pytest.mark.parametrize("mode", ["minmax", "rrf"])
def test_cut_quirk_an_item_first_seen_beyond_the_cut_is_a_miss(gpu, mode):
    """Full overlap, cut = 520, alpha = 1: the order follows list a, where an item's two entries tie and
    sit side by side, so the first entry beyond the cut has about 260 distinct ids before it; it is a
    miss at k = 500 all the same, and a hit once the cut is lifted."""
    vecs, cand = _vectors("gaussian"), _pool(2000, "full")
    _, _, sa, sb = _run(gpu, vecs, cand, [set()] * Q, [1.0], mode, 520, [500])
    wa, wb = REF.fusion_weights([1.0])
    truth = []
    for q in range(Q):
        na, nb = REF.normalise(sa[q], mode, 200.0), REF.normalise(sb[q], mode, 200.0)
        ids = cand[q][REF.order_desc((wa[0] * na + wb[0] * nb).astype(np.float32))]
        head = set(ids[:520].tolist())
        j = next(j for j in range(520, 2000) if ids[j] not in head)
        assert len(set(ids[:j].tolist())) < 500
        truth.append({int(ids[j])})
    hits, _, _, _ = _downstream(gpu, vecs, cand, truth, [1.0], mode, 520)
    assert not hits.any()
    hits, _, _, _ = _downstream(gpu, vecs, cand, truth, [1.0], mode, 2000)
    assert (hits[:, 0] & (1 << _ks(2000, 2000).index(500))).all()


@pytest.mark.parametrize("mode", ["minmax", "rrf"])
def test_a_constant_list_leaves_the_order_to_the_other(gpu, mode):
    ua, Ia, ub, Ib = _vectors("gaussian")
    vecs = (np.zeros_like(ua), Ia, ub, Ib)   # every score of list a is 0
    cand = _pool(128, "partial")
    _, lists, sa, _ = _downstream(gpu, vecs, cand, _truth(cand), ALPHAS[11], mode, 128)
    assert not sa.any()
    if mode == "minmax":   # na = 0 everywhere: alpha = 1 keeps the pool's own order
        for q in range(Q):
            first = list(dict.fromkeys(cand[q].tolist()))[:lists.shape[2]]
            assert lists[q, 0, :len(first)].tolist() == first


@pytest.mark.parametrize("C", [3, 2000, 2048])
@pytest.mark.parametrize("mode", ["minmax", "rrf"])
def test_exact_grid_inputs_agree_end_to_end(gpu, mode, C):
    """Entries are multiples of 2^-4 in [-1, 1]: products are multiples of 2^-8, a 128-term sum stays
    below 2^7, so every partial sum fits fp32's 24 bits and the dot product is exact in any order."""
    vecs = _vectors("grid")
    ua, Ia, ub, Ib = vecs
    cand = _pool(C, "partial")
    truth, alphas, cut = _truth(cand, seed=1), ALPHAS[11], min(C, 520)
    ks = _ks(C, cut)
    hits, lists, sa, sb = _run(gpu, vecs, cand, truth, alphas, mode, cut, ks)
    ra = np.stack([(Ia[cand[q]].astype(np.float64) @ ua[q].astype(np.float64)) for q in range(Q)]).astype(np.float32)
    rb = np.stack([(Ib[cand[q]].astype(np.float64) @ ub[q].astype(np.float64)) for q in range(Q)]).astype(np.float32)
    assert np.array_equal(sa, ra) and np.array_equal(sb, rb)
    wa, wb = REF.fusion_weights(alphas)
    rh, rl = REF.fuse_rank(ra, rb, cand, wa, wb, mode, 200.0, cut, ks, truth)
    assert np.array_equal(lists, rl) and np.array_equal(hits, rh)
    assert hits.any()   # the case is not vacuous: some user hits


def test_a_pool_entry_outside_the_corpus_sets_the_flag(gpu):
    ua, Ia, ub, Ib = (torch.tensor(t).to(gpu) for t in _vectors("grid"))
    cand = torch.tensor(_pool(128, "none")).to(gpu)
    cand[2, 5] = NI
    cand[4, 0] = -3
    off, tr = MI.truth_csr({q: set() for q in range(Q)}, list(range(Q)), NI)
    out = ops.fuse_rank(ua, Ia, ub, Ib, cand, [0.5], [5], torch.tensor(off).to(gpu), torch.tensor(tr).to(gpu),
                        return_scores=True)
    assert out.flag.item() == 1
    assert out.sa[2, 5].item() == 0.0 and out.sb[4, 0].item() == 0.0
