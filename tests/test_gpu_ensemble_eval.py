"""tower_code.mined_inference on the device against tests/ensemble_ref.py: the three evaluators on
exact-grid vectors (every dot product exact in fp32 in any order, so torch.matmul, the kernels and
numpy see the same scores, ties included), users in several batches, then one run on Gaussian rows
through the normalisation, and ops.first_hit against a Python set scan."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import recsys_amd  # noqa: F401
from recsys_amd import ops
from recsys_amd.tower_code import mined_inference as MI
from tests import ensemble_ref as REF

pytestmark = pytest.mark.gpu

N_USERS, N_ITEMS, D_SEQ, D_GNN = 300, 5000, 128, 64
K_LIST = [5, 20, 100]
REF_CACHE = {}   # per user: the reference's score rows and their orders, shared by every evaluation below


@functools.lru_cache(maxsize=None)
def _grid():
    """Vectors with entries k / 16 in [-1, 1] and a ground truth: a third of the users without items, the
    rest with up to four random items and, two in three of those, one item from near the top of a list."""
    rng = np.random.default_rng(11)
    make = lambda n, d: (rng.integers(-16, 17, size=(n, d)) / 16.0).astype(np.float32)
    su, si, gu, gi = make(N_USERS + 20, D_SEQ), make(N_ITEMS, D_SEQ), make(N_USERS + 20, D_GNN), make(N_ITEMS, D_GNN)
    gt = {}
    for u in rng.permutation(N_USERS + 20)[:N_USERS].tolist():   # the user rows are neither sorted nor dense
        items = set() if u % 3 == 0 else set(rng.integers(0, N_ITEMS, size=int(rng.integers(1, 5))).tolist())
        if u % 3 == 1:
            scores = (gi @ gu[u]) if u % 2 else (si @ su[u])
            items.add(int(np.argsort(-scores, kind="stable")[int(rng.integers(0, 150))]))
        gt[u] = items
    return su, si, gu, gi, gt


def _dev(gpu):
    su, si, gu, gi, gt = _grid()
    return [torch.tensor(t).to(gpu) for t in (su, si, gu, gi)], gt


def _same(got, want):
    assert got["users"] == want["users"] == N_USERS
    assert got["hits"] == want["hits"]
    assert got["best_alpha"] == want["best_alpha"]
    assert got["recall"] == want["recall"]
    assert list(got["hits"]) == list(want["hits"])


@pytest.mark.parametrize("pool", [200, 1000])
@pytest.mark.parametrize("mode", ["minmax", "rrf"])
def test_fused_evaluators_equal_the_reference(gpu, mode, pool):
    su, si, gu, gi, gt = _grid()
    (dsu, dsi, dgu, dgi), _ = _dev(gpu)
    if mode == "minmax":
        got = MI.evaluate_weighted_score_ensemble(dsu, dsi, dgu, dgi, gt, gpu, k_list=K_LIST, batch_size=128,
                                                  candidate_pool_size=pool, assume_normalized=True)
    else:
        got = MI.evaluate_rrf_ensemble(dsu, dsi, dgu, dgi, gt, gpu, k_list=K_LIST, batch_size=128,
                                       candidate_pool_size=pool, k_rrf=200, assume_normalized=True)
    want = REF.evaluate_fused(su, si, gu, gi, gt, K_LIST, 0.1, pool, mode, k_rrf=200, cache=REF_CACHE)
    _same(got, want)
    assert len(got["hits"]) == 11 and sum(got["hits"][0.5].values()) > 0


def test_ratio_merge_evaluator_equals_the_reference(gpu):
    su, si, gu, gi, gt = _grid()
    (dsu, dsi, dgu, dgi), _ = _dev(gpu)
    got = MI.evaluate_multi_vector_ensemble(dsu, dsi, dgu, dgi, gt, gpu, k_list=K_LIST, batch_size=128,
                                            assume_normalized=True)
    want = REF.evaluate_multi_vector(su, si, gu, gi, gt, K_LIST, 0.2, cache=REF_CACHE)
    _same(got, want)
    assert len(got["hits"]) == 6 and sum(got["hits"][1.0].values()) > 0


def test_gaussian_rows_run_through_the_normalisation(gpu):
    g = torch.Generator().manual_seed(5)
    su, si = torch.randn(200, D_SEQ, generator=g).to(gpu), torch.randn(N_ITEMS, D_SEQ, generator=g).to(gpu)
    gu, gi = torch.randn(200, D_GNN, generator=g).to(gpu), torch.randn(N_ITEMS, D_GNN, generator=g).to(gpu)
    top = torch.topk(F.normalize(gu) @ F.normalize(gi).T, 3, dim=1).indices.cpu().tolist()
    gt = {u: ({top[u][2]} if u % 2 else {int(u * 7 % N_ITEMS)}) for u in range(200)}
    for res, n_alpha in ((MI.evaluate_weighted_score_ensemble(su, si, gu, gi, gt, gpu, k_list=K_LIST, batch_size=128), 11),
                         (MI.evaluate_rrf_ensemble(su, si, gu, gi, gt, gpu, k_list=K_LIST, batch_size=128), 11),
                         (MI.evaluate_multi_vector_ensemble(su, si, gu, gi, gt, gpu, k_list=K_LIST, batch_size=128), 6)):
        assert set(res) == {"best_alpha", "hits", "recall", "users"} and res["users"] == 200
        assert len(res["hits"]) == n_alpha and res["best_alpha"] in res["hits"]
        for a in res["hits"]:
            assert list(res["hits"][a]) == K_LIST
            assert all(0.0 <= res["recall"][a][k] <= 1.0 for k in K_LIST)
            assert all(res["recall"][a][k] == res["hits"][a][k] / 200 for k in K_LIST)
        # scaling a row does not move its cosine order: the GNN retriever alone finds its own third-best item
        assert res["hits"][1.0][5] >= 100


def test_first_hit_equals_a_set_scan(gpu):
    rng = np.random.default_rng(3)
    Qn, K = 70, 333
    lists = rng.integers(0, 400, size=(Qn, K)).astype(np.int32)
    lists[5] = -1   # a padded list
    truth = [set(rng.integers(0, 4000 if q % 2 else 400, size=q % 9 * (40 if q % 4 == 0 else 1)).tolist())
             for q in range(Qn)]
    off, tr = MI.truth_csr(dict(enumerate(truth)), list(range(Qn)))
    want = REF.first_hit(lists, truth)
    assert (want == K).any() and (want == 0).any() and ((want > 0) & (want < K)).any()
    d_off, d_tr = torch.tensor(off).to(gpu), torch.tensor(tr).to(gpu)
    got = ops.first_hit(torch.tensor(lists).to(gpu), d_off, d_tr)
    assert got.dtype == torch.int32 and got.cpu().numpy().tolist() == want.tolist()
    got64 = ops.first_hit(torch.tensor(lists.astype(np.int64)).to(gpu), d_off, d_tr)   # retrieve_topk's index type
    assert torch.equal(got, got64)
