"""gnn_model.v1_lightgcl.LightGCL on the device against the float64 reference of tests/lightgcl_ref.py:
both views of forward() within their composed per-element bounds; the loss terms within 1e-5 relative
and both tables' gradients within 1e-4 of each gradient's max (the project's oracle tolerances for
losses and gradients), for the forward()-based composition and for train_step's row-restricted path;
bit-reproducible steps; three Adam steps tracking float64 within 1e-5 wherever the gradient is resolved
(oracle/agreement.py's rule); the evaluation's hit counts against a dense float64 top-k.

Seeded power-law graph (3001 users, 500 items, ~20k edges, several rows past the chunk length), D = 64,
2 layers, q = 5 with U, S, V handed to the model explicitly (a seeded float64 svd_lowrank in the set-up:
the model itself draws nothing), a batch of 257 triples with repeated users and items."""
import functools

import numpy as np
import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import ops
from recsys_amd.gnn_model import v1_evaluate_lightgcl as EV
from recsys_amd.gnn_model import v1_lightgcl as G
from tests import lightgcl_ref as REF

pytestmark = pytest.mark.gpu

NU, NI, B = 3001, 500, 257
CFG = {"emb_dim": 64, "n_layers": 2, "temp": 0.2, "lambda_ssl": 0.01, "lambda_reg": 1e-5}
LOSS_RTOL, GRAD_TOL, PARAM_TOL, LR = 1e-5, 1e-4, 1e-5, 1e-3


def _svd(A, q):
    U, S, Vh = torch.linalg.svd(A)
    return U[:, :q].float().contiguous(), S[:q].float().contiguous(), Vh[:q].t().float().contiguous()


@functools.lru_cache(maxsize=None)
def _setup():
    adj = G.NormAdjacency(REF.power_law_edges(NU, NI), NU, NI)
    A = REF.dense_norm(adj)
    torch.manual_seed(1234)   # seeded set-up of the factors handed to the model, which draws nothing itself
    U, S, V = (t.float().contiguous() for t in torch.svd_lowrank(A, q=5, niter=2))
    torch.manual_seed(0)
    model = G.LightGCL(NU, NI, CFG, adj, (U, S, V))
    state = {k: v.clone() for k, v in model.state_dict().items()}
    return adj, A, (U, S, V), state


@functools.lru_cache(maxsize=None)
def _batch(seed):
    g = torch.Generator().manual_seed(100 + seed)
    users = torch.randint(0, NU, (B,), generator=g)
    pos = torch.randint(0, NI, (B,), generator=g)
    neg = torch.randint(0, NI, (B,), generator=g)
    users[:40] = users[40:80]          # repeated users
    pos[:30] = pos[100:130]            # repeated items (beside the Zipf-free draw's own repeats)
    neg[:10] = pos[:10]
    assert torch.unique(users).numel() < B and torch.unique(pos).numel() < B
    return users, pos, neg


def _model(gpu, cfg=None):
    adj, _, svd, state = _setup()
    model = G.LightGCL(NU, NI, cfg or CFG, adj, svd)
    model.load_state_dict(state)
    return model.to(gpu)


@functools.lru_cache(maxsize=None)
def _reference(lambda_ssl):
    """Three float64 Adam steps from the initial state on batches 0, 1, 2 (step 0 is also the
    reference of the single-step tests)."""
    _, A, (U, S, V), state = _setup()
    cfg = dict(CFG, lambda_ssl=lambda_ssl)
    return REF.train(state["embedding_user.weight"], state["embedding_item.weight"], A, U.double(), S.double(),
                     V.double(), cfg, [_batch(0), _batch(1), _batch(2)] if lambda_ssl == CFG["lambda_ssl"]
                     else [_batch(0)], LR)


def _within(got, want, bound, what):
    err = (got.detach().cpu().double() - want).abs()
    over = err > bound
    assert not bool(over.any()), (f"{what}: {int(over.sum())} elements over their bound, worst "
                                  f"{float((err / bound.clamp(min=1e-300))[over].max()):.3g} x bound")


def _check_losses(got, want, what):
    got = [float(g.detach()) if torch.is_tensor(g) else float(g) for g in got]
    for name, g, w in zip(("bpr", "ssl", "reg", "total"), got, want):
        print(f"{what} {name}: got {g:.9g} f64 {w:.9g} rel {abs(g - w) / abs(w):.3g}")
    for name, g, w in zip(("bpr", "ssl", "reg", "total"), got, want):
        assert abs(g - w) <= LOSS_RTOL * abs(w), (what, name, g, w)


def _check_grads(model, want, what):
    got = (model.embedding_user.weight.grad, model.embedding_item.weight.grad)
    errs = []
    for name, g, w in zip(("embedding_user", "embedding_item"), got, want):
        scale = float(w.abs().max())
        errs.append(float((g.cpu().double() - w).abs().max()) / scale)
        print(f"{what} grad {name}: max err / max |f64 grad| = {errs[-1]:.3g}")
    assert max(errs) <= GRAD_TOL, (what, errs)


def test_forward_views_against_float64(gpu):
    _, A, (U, S, V), state = _setup()
    E = torch.cat([state["embedding_user.weight"], state["embedding_item.weight"]]).double()
    model = _model(gpu)
    with torch.no_grad():
        local, glob = model()
    assert local.shape == glob.shape == (NU + NI, 64)
    _within(local, REF.local_view(A, E, 2), REF.local_view_bound(A, E, 2), "local_final")
    _within(glob, REF.global_view(U.double(), S.double(), V.double(), E, 2), REF.global_view_bound(U, S, V, E, 2),
            "global_final")


@pytest.mark.parametrize("lambda_ssl", [CFG["lambda_ssl"], 1.0])
def test_forward_composition_losses_and_gradients(gpu, lambda_ssl):
    ref = _reference(lambda_ssl)[0]
    model = _model(gpu, dict(CFG, lambda_ssl=lambda_ssl))
    users, pos, neg = (t.to(gpu) for t in _batch(0))
    local, glob = model()
    bpr = model.calc_bpr_loss(local, users, pos + NU, neg + NU)
    ssl = model.calc_ssl_loss(local, glob, users, pos + NU)
    reg = model.get_l2_reg(users, pos, neg)
    total = bpr + lambda_ssl * ssl + CFG["lambda_reg"] * reg
    total.backward()
    _check_losses((bpr, ssl, reg, total), ref["losses"], f"forward() lambda_ssl={lambda_ssl}")
    _check_grads(model, ref["grads"], f"forward() lambda_ssl={lambda_ssl}")


@pytest.mark.parametrize("lambda_ssl", [CFG["lambda_ssl"], 1.0])
def test_train_step_losses_and_gradients(gpu, lambda_ssl):
    ref = _reference(lambda_ssl)[0]
    model = _model(gpu, dict(CFG, lambda_ssl=lambda_ssl))
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    bpr, ssl, reg = model.train_step(*(t.to(gpu) for t in _batch(0)), opt)
    assert bpr.device.type == "cuda" and not bpr.requires_grad
    total = float(bpr) + lambda_ssl * float(ssl) + CFG["lambda_reg"] * float(reg)
    _check_losses((bpr, ssl, reg, total), ref["losses"], f"train_step lambda_ssl={lambda_ssl}")
    _check_grads(model, ref["grads"], f"train_step lambda_ssl={lambda_ssl}")


def test_propagate_backward_is_its_forward_bit_for_bit(gpu):
    adj = _setup()[0].to(gpu)
    g = torch.Generator().manual_seed(9)
    E = torch.randn(adj.n, 64, generator=g).to(gpu).requires_grad_(True)
    cot = torch.randn(adj.n, 64, generator=g).to(gpu)
    ops.lightgcl_propagate(E, adj, 2).backward(cot)
    assert torch.equal(E.grad, ops.lightgcl_propagate(cot, adj, 2))


@pytest.mark.parametrize("n_layers", [0, 1, 3])
def test_other_layer_counts_on_a_small_graph(gpu, n_layers):
    edges = torch.tensor([[4, 0, 3, 0, 2, 4, 1], [2, 3, 0, 1, 2, 0, 3]])
    adj = G.NormAdjacency(edges, 5, 4)
    A = REF.dense_norm(adj)
    U, S, V = _svd(A, 3)
    torch.manual_seed(1)
    model = G.LightGCL(5, 4, dict(CFG, n_layers=n_layers), adj, (U, S, V)).to(gpu)
    E = torch.cat([model.embedding_user.weight, model.embedding_item.weight]).detach().cpu().double()
    local, glob = model()
    _within(local, REF.local_view(A, E, n_layers), REF.local_view_bound(A, E, n_layers), "local_final")
    _within(glob, REF.global_view(U.double(), S.double(), V.double(), E, n_layers),
            REF.global_view_bound(U, S, V, E, n_layers), "global_final")
    g = torch.Generator().manual_seed(2)
    c1, c2 = torch.randn(9, 64, generator=g), torch.randn(9, 64, generator=g)
    ((local * c1.to(gpu)).sum() + (glob * c2.to(gpu)).sum()).backward()
    Er = E.clone().requires_grad_(True)
    ((REF.local_view(A, Er, n_layers) * c1).sum()
     + (REF.global_view(U.double(), S.double(), V.double(), Er, n_layers) * c2).sum()).backward()
    got = torch.cat([model.embedding_user.weight.grad, model.embedding_item.weight.grad]).cpu().double()
    assert float((got - Er.grad).abs().max()) <= GRAD_TOL * float(Er.grad.abs().max())


def test_train_step_is_bit_reproducible(gpu):
    runs = []
    for _ in range(2):
        model = _model(gpu)
        opt = torch.optim.Adam(model.parameters(), lr=LR)
        losses = model.train_step(*(t.to(gpu) for t in _batch(0)), opt)
        runs.append([t.clone() for t in losses] + [p.grad.clone() for p in model.parameters()]
                    + [p.detach().clone() for p in model.parameters()])
    for a, b in zip(*runs):
        assert torch.equal(a, b)


def test_three_adam_steps_track_float64(gpu):
    """Three train_steps (Adam, lr 1e-3, three different batches) against three float64 Adam steps:
    parameters within 1e-5 wherever the gradient is resolved, i.e. wherever no step's float64 gradient
    lies within the allowed gradient error (1e-4 of that step's max) of zero."""
    ref = _reference(CFG["lambda_ssl"])
    model = _model(gpu)
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    for s in range(3):
        model.train_step(*(t.to(gpu) for t in _batch(s)), opt)
    for k, p in enumerate((model.embedding_user.weight, model.embedding_item.weight)):
        # unresolved: the float64 gradient of some step lies within the allowed gradient error of zero
        unres = torch.zeros(p.shape, dtype=torch.bool)
        for step in ref:
            gr = step["grads"][k]
            unres |= gr.abs() <= GRAD_TOL * float(gr.abs().max())
        diff = (p.detach().cpu().double() - ref[2]["params"][k]).abs()
        moved = (ref[2]["params"][k] - _setup()[3][("embedding_user.weight", "embedding_item.weight")[k]].double()).abs()
        print(f"table {k}: resolved {int((~unres).sum())} of {unres.numel()}, worst resolved diff "
              f"{float(diff[~unres].max()):.3g}, worst diff {float(diff.max()):.3g}, largest move {float(moved.max()):.3g}")
        assert int((~unres).sum()) > 1000
        assert float(diff[~unres].max()) <= PARAM_TOL


def test_evaluate_recall_against_dense_float64(gpu):
    nu, ni = 120, 300
    g = torch.Generator().manual_seed(4)
    edges = torch.stack([torch.randint(0, nu, (500,), generator=g), torch.randint(0, ni, (500,), generator=g)])
    adj, U, S, V = G.build_graph(edges, nu, ni, "cpu", q=5)
    model = G.LightGCL(nu, ni, CFG, adj, (U, S, V))
    with torch.no_grad():   # dyadic values: every dot product is exact in any accumulation order
        model.embedding_user.weight.copy_(torch.randint(-8, 9, (nu, 64), generator=g) / 8.0)
        model.embedding_item.weight.copy_(torch.randint(-8, 9, (ni, 64), generator=g) / 8.0)
        model.embedding_item.weight[0] = 0.0   # the padding row would win every query if it were scored
        model.embedding_user.weight[:, 0] = 1.0
        model.embedding_item.weight[:, 0] = -1.0
        model.embedding_item.weight[0, 0] = 64.0
    model = model.to(gpu)
    rng = np.random.default_rng(0)
    truth = {int(u): set(int(i) for i in rng.choice(np.arange(1, ni), size=3, replace=False))
             for u in rng.choice(nu, size=100, replace=False)}
    k_list = [5, 20]
    out = EV.evaluate_recall(model, truth, gpu, k_list=k_list, batch_size=32)
    scores = (model.embedding_user.weight.detach().cpu().double()
              @ model.embedding_item.weight.detach().cpu().double().t()).numpy()
    assert scores[:, 0].min() > scores[:, 1:].max()
    scores[:, 0] = -np.inf
    hits = {k: 0 for k in k_list}
    for u, items in truth.items():
        order = np.lexsort((np.arange(ni), -scores[u]))   # score descending, ties to the lower index
        for k in k_list:
            hits[k] += not items.isdisjoint(order[:k].tolist())
    assert out["hits"] == hits and out["users"] == 100
    assert out["recall"] == {k: hits[k] / 100 for k in k_list}
    top = EV.topk_items(model.embedding_user.weight.data, model.embedding_item.weight.data, 20)
    assert int(top.min()) >= 1 and int(top.max()) < ni
    assert np.array_equal(top.cpu().numpy(), np.stack([np.lexsort((np.arange(ni), -scores[u]))[:20]
                                                       for u in range(nu)]))
    users_f, items_f = EV.compute_final_embeddings(model, model.adj, n_layers=2)
    assert users_f.shape == (nu, 64) and items_f.shape == (ni, 64)
    rows = torch.tensor([0, nu, nu + ni - 1, 0], device=gpu)
    assert torch.equal(EV.compute_final_embeddings(model, model.adj, 2, rows=rows),
                       torch.cat([users_f, items_f])[rows])


def test_svd_lowrank_of_k34_on_the_device(gpu):
    edges = torch.tensor([[u for u in range(3) for _ in range(4)], [i for _ in range(3) for i in range(4)]])
    torch.manual_seed(0)
    adj, U, S, V = G.build_graph(edges, 3, 4, gpu, q=5)
    assert U.device.type == "cuda" and adj.device.type == "cuda"
    dense = REF.dense_norm(adj).float()
    assert torch.allclose((U @ torch.diag(S) @ V.t()).cpu(), dense, atol=1e-4)
    assert torch.equal(adj.K, V.t() @ U)
