"""ops.retrieve_topk for 512 < k <= 2048: the bf16 single scan with the larger margin set, its exact
fallback for listed queries (fp32 score rows in a bounded scratch + a radix select per row), the
materialised route on corpora the scan's plan does not serve, and k <= 512 on the shared code.

Sizes: 64 queries and, per k, the smallest corpus at which rsx_topk_path answers 2 (asked of the
library, not hard-coded) plus 37 items, so that the last tile and the last split are ragged. The
float64 / fp32 oracles (oracle.retrieval) are computed once per input and shared.

Criteria: dyadic inputs (every score exact in fp32 and in the bf16 image) must equal the float64 oracle
bit for bit, indices and scores; spread unit vectors are held to the near-tie criterion of
tests/test_gpu_retrieval_1m.py, restated in _check_near_ties. The fallback counts are printed
(pytest -s) and summarised in DESIGN.md, section 4.
"""
import functools

import pytest
import torch
import torch.nn.functional as F

import recsys_amd  # noqa: F401
from recsys_amd import _native as N
from recsys_amd import ops
from oracle import retrieval as OR

pytestmark = pytest.mark.gpu

Q = 64


@functools.lru_cache(maxsize=None)
def _fused_ni(k, q=Q):
    """The smallest item count at which the library serves k on the fused path (monotone in NI), + 37."""
    lib = N.lib()
    lo, hi = k, 1 << 24                      # path(lo) may be anything; path(hi) == 2
    assert lib.rsx_topk_path(q, hi, k) == 2
    while lo < hi:
        mid = (lo + hi) // 2
        if lib.rsx_topk_path(q, mid, k) == 2:
            hi = mid
        else:
            lo = mid + 1
    assert lib.rsx_topk_path(q, lo, k) == 2 and lib.rsx_topk_path(q, lo - 1, k) != 2
    return lo + 37


@functools.lru_cache(maxsize=None)
def _dyadic(seed, n_items, q=Q):
    g = torch.Generator().manual_seed(seed)
    U = torch.randint(-4, 5, (q, 128), generator=g).float() / 8.0
    I = torch.randint(-4, 5, (n_items, 128), generator=g).float() / 8.0
    return U, I


@functools.lru_cache(maxsize=None)
def _spread(seed, n_items, q=Q):
    g = torch.Generator().manual_seed(seed)
    U = F.normalize(torch.randn(q, 128, generator=g), dim=1)
    I = F.normalize(torch.randn(n_items, 128, generator=g), dim=1)
    return U, I


def _exact_scores(U, I, idx):
    """float64 scores of the items idx [Q, k] for each query."""
    return torch.einsum("qkd,qd->qk", I[idx].double(), U.double())


def _check_near_ties(U, I, k, s, i):
    """s, i: the HIP result (CPU). With eps = the fp32 rounding bound of a 128-term dot product: k distinct
    in-range indices per query; scores sorted; each returned score within eps of the float64 score of its
    item; rank-wise within 2 eps of the exact ranking; every index that differs from the fp32 oracle's
    within 4 eps of it; fewer than 1 % of the places differ."""
    n_items = I.shape[0]
    eps = OR.fp32_dot_bound(128, U.norm(dim=1).max().item(), I.norm(dim=1).max().item())
    assert (i >= 0).all() and (i < n_items).all()
    assert all(row.unique().numel() == k for row in i)
    assert (s[:, :-1] >= s[:, 1:]).all()
    ours = _exact_scores(U, I, i)
    assert (s.double() - ours).abs().max().item() <= eps
    rs64, _ = OR.retrieve_topk_chunked(U, I, k, dtype=torch.float64)
    assert (ours - rs64).abs().max().item() <= 2 * eps
    _, ri32 = OR.retrieve_topk_chunked(U, I, k, dtype=torch.float32)
    mism = i != ri32
    ref = _exact_scores(U, I, ri32)
    if mism.any():
        assert (ours - ref).abs()[mism].max().item() <= 4 * eps
    frac = mism.float().mean().item()
    assert frac < 0.01, frac
    return frac, eps


def _check_bit_exact(U, I, k, s, i):
    rs, ri = OR.retrieve_topk_chunked(U, I, k, dtype=torch.float64)
    assert torch.equal(i.cpu(), ri)
    assert torch.equal(s.cpu().double(), rs)


@pytest.mark.parametrize("k,q", [(513, Q), (1000, Q), (2048, Q), (1000, 130)])
def test_large_k_dyadic_bit_exact(gpu, k, q):
    """Heavy exact ties at the k-th score; q = 130 puts two rows into a second 128-row block."""
    U, I = _dyadic(100 + k + q, _fused_ni(k, q), q)
    diag = {}
    s, i = ops.retrieve_topk(U.to(gpu), I.to(gpu), k, diag=diag)
    print(f"[dyadic k={k} q={q} NI={I.shape[0]}] exact-kernel queries {diag['fallback_queries']}/{q}")
    assert diag["path"] == "bf16"
    _check_bit_exact(U, I, k, s, i)


@pytest.mark.parametrize("k", [1000, 2048])
def test_large_k_spread_near_ties(gpu, k):
    U, I = _spread(200 + k, _fused_ni(k))
    diag = {}
    s, i = ops.retrieve_topk(U.to(gpu), I.to(gpu), k, diag=diag)
    assert diag["path"] == "bf16"
    frac, eps = _check_near_ties(U, I, k, s.cpu(), i.cpu())
    print(f"[spread k={k} NI={I.shape[0]}] exact-kernel queries {diag['fallback_queries']}/{Q}, "
          f"index mismatches vs the fp32 oracle {frac:.5f} (all within 4 eps = {4 * eps:.2e})")
    assert diag["fallback_queries"] <= Q // 8       # a path that falls back for most queries is not the feature


def _scattered_copies(seed, n_items, n_copies, rows):
    """Dyadic queries; items scaled by 1/64 (they score far lower) except, for each query r of `rows`,
    n_copies exact copies of it at positions of its own (one permutation cut into disjoint pieces)."""
    g = torch.Generator().manual_seed(seed)
    U = torch.randint(-4, 5, (Q, 128), generator=g).float() / 8.0
    I = torch.randint(-4, 5, (n_items, 128), generator=g).float() / 512.0
    perm = torch.randperm(n_items, generator=g)
    assert len(rows) * n_copies <= n_items
    pos = {}
    for t, r in enumerate(rows):
        pos[r] = perm[t * n_copies:(t + 1) * n_copies].sort().values
        I[pos[r]] = U[r]
    return U, I, pos


def test_large_k_all_tied_margin_no_fallback(gpu):
    """k + (margin capacity - k) // 2 exact copies of every query, scattered: the whole margin set ties, the
    rescored set is sorted by index alone, and no query leaves the fused path. 64 x 2548 disjoint positions
    do not fit the smallest fused corpus (131,109 items), so this case runs at four times that size."""
    k = 1000
    n_copies = k + (N.lib().rsx_topk_margin_capacity(k) - k) // 2
    n_items = 4 * (_fused_ni(k) - 37) + 37
    U, I, pos = _scattered_copies(31, n_items, n_copies, list(range(Q)))
    diag = {}
    s, i = ops.retrieve_topk(U.to(gpu), I.to(gpu), k, diag=diag)
    assert diag["path"] == "bf16" and diag["fallback_queries"] == 0
    want = torch.stack([pos[r][:k] for r in range(Q)])
    assert torch.equal(i.cpu(), want)
    assert (s.cpu() == (U * U).sum(dim=1, keepdim=True)).all()


def test_large_k_forced_exact_fallback(gpu):
    """More exact copies than the margin set holds, for 4 of the 64 queries: those four are listed and served
    by the exact fallback (the k lowest copy positions), the rest stay on the fused path, and all 64 equal the
    float64 oracle bit for bit. The four queries live on columns 0..63 and the other sixty on columns
    64..127, so a copy scores exactly 0 for every other query and never crowds its margin set."""
    k = 1000
    n_items = _fused_ni(k)
    n_copies = N.lib().rsx_topk_margin_capacity(k) + 200
    assert n_copies <= N.lib().rsx_topk_entry_capacity()      # the margin set overflows, not the entry buffer
    g = torch.Generator().manual_seed(41)
    U = torch.randint(-4, 5, (Q, 128), generator=g).float() / 8.0
    U[:4, 64:] = 0.0
    U[4:, :64] = 0.0
    I = torch.randint(-4, 5, (n_items, 128), generator=g).float() / 512.0
    perm = torch.randperm(n_items, generator=g)
    pos = [perm[r * n_copies:(r + 1) * n_copies].sort().values for r in range(4)]
    for r in range(4):
        I[pos[r]] = U[r]
    diag = {}
    s, i = ops.retrieve_topk(U.to(gpu), I.to(gpu), k, diag=diag)
    print(f"[forced fallback k={k} NI={n_items}] exact-kernel queries {diag['fallback_queries']}/{Q}")
    assert diag["path"] == "bf16" and 4 <= diag["fallback_queries"] < Q // 2
    assert torch.equal(i[:4].cpu(), torch.stack([p[:k] for p in pos]))
    _check_bit_exact(U, I, k, s, i)


def test_large_k_contiguous_cluster_fallback(gpu):
    """1,500 near-copies of each of four queries stored contiguously: they fall into three or four lane
    streams of 512 items, far beyond a stream's capacity, so those queries are listed. A near-copy is
    normalize(u_c + 0.02 n): for another query u' it scores about cos(u', u_c) +- 0.02, so u' overflows a
    stream too only if more than 6 % of a cluster clears its k-th score (~0.215 here), i.e. cos(u', u_c) >
    ~0.19, 2.1 sigma of a random pair: about 4 further queries are expected, well below Q // 4."""
    k, n_near = 1000, 1500
    assert n_near > 4 * N.lib().rsx_topk_stream_capacity()
    n_items = _fused_ni(k)
    U, I = (t.clone() for t in _spread(300, n_items))
    g = torch.Generator().manual_seed(301)
    for c in range(4):
        lo = 50_000 + n_near * c
        I[lo:lo + n_near] = F.normalize(U[c] + 0.02 * torch.randn(n_near, 128, generator=g), dim=1)
    diag = {}
    s, i = ops.retrieve_topk(U.to(gpu), I.to(gpu), k, diag=diag)
    print(f"[clustered k={k} NI={n_items}] exact-kernel queries {diag['fallback_queries']}/{Q}")
    assert diag["path"] == "bf16" and 4 <= diag["fallback_queries"] < Q // 4
    _check_near_ties(U, I, k, s.cpu(), i.cpu())
    for c in range(4):                                         # each cluster fills its query's top-k
        lo = 50_000 + n_near * c
        assert (i[c].cpu() >= lo).all() and (i[c].cpu() < lo + n_near).all()


@pytest.mark.parametrize("k", [1000, 2048])
def test_large_k_materialised_route(gpu, k):
    """A 5000-item corpus is below every fused plan for k > 512: score chunks + select_topk_rows."""
    for kind, data in (("spread", _spread(400 + k, 5000)), ("dyadic", _dyadic(500 + k, 5000))):
        U, I = data
        diag = {}
        s, i = ops.retrieve_topk(U.to(gpu), I.to(gpu), k, diag=diag)
        assert diag == {"path": "materialised", "fallback": False, "fallback_queries": 0}
        assert s.dtype == torch.float32 and i.dtype == torch.int64 and s.shape == i.shape == (Q, k)
        if kind == "spread":
            _check_near_ties(U, I, k, s.cpu(), i.cpu())
        else:
            _check_bit_exact(U, I, k, s, i)


def test_large_k_cached_corpus_follows_updates(gpu):
    """Two calls on one corpus, then an in-place row update that creates a new winner: the cached bf16 image
    is rebuilt (tests/test_gpu_retrieval_1m.py::test_retrieval_cached_corpus_follows_updates at k = 1000)."""
    k = 1000
    U, I = _dyadic(600, _fused_ni(k))
    U, I = U.to(gpu), I.to(gpu).clone()
    for step in range(3):
        s, i = ops.retrieve_topk(U, I, k)
        _check_bit_exact(U.cpu(), I.cpu(), k, s, i)
        if step == 1:
            I[123] = 2.0 * U[0]                  # in place: a new winner for query 0
        elif step == 2:
            assert i[0, 0].item() == 123
    assert ops._TOPK_CORPUS[gpu]["key"].matches([I])


def test_k_500_unchanged_on_the_shared_code(gpu):
    """k <= 512 at the same corpus size: the assertions of the 1M tests (bit-exact on dyadic data; the
    near-tie criterion and a rare fallback on spread data)."""
    k, n_items = 500, _fused_ni(1000)
    U, I = _dyadic(700, n_items)
    diag = {}
    s, i = ops.retrieve_topk(U.to(gpu), I.to(gpu), k, diag=diag)
    assert diag["path"] == "bf16"
    _check_bit_exact(U, I, k, s, i)
    U, I = _spread(701, n_items)
    s, i = ops.retrieve_topk(U.to(gpu), I.to(gpu), k, diag=diag)
    assert diag["path"] == "bf16"
    _check_near_ties(U, I, k, s.cpu(), i.cpu())
    assert diag["fallback_queries"] <= Q // 64
