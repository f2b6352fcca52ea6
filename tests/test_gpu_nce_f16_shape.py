"""The f16 grouped kernels at the edges of their 16x16x32 MFMA blocks (csrc/nce_grouped_f16.hip: the
column pass holds two 16-column owner halves per wave and takes each 32-row streamed tile as two
16-row halves).

Reference and criteria are those of tests/test_gpu_nce_paths.py (its problem / run_grouped / check):
the float64 restatement on the CPU, mean loss within 1e-4, each gradient within 1e-3 of its
reference's max-abs. Precision "f16" only, with the fused row gradient on. Every shape is a fraction
of a second; the references are computed once per shape and never modified."""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import recsys_amd  # noqa: F401
from recsys_amd import ops
from tests import test_gpu_nce_paths as paths
from tests.test_gpu_kernels import _nce_rows_ref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (n_users, max_len, n_items, seed) -> (N, D). D on and around the owner halves' 16-column edges
# (N = 235: eight tiles, the last with 11 rows) ...
D_EDGES = {
    (20, 20, 15, 0): (235, 15),
    (20, 20, 16, 0): (235, 16),
    (20, 20, 17, 0): (235, 17),
    (20, 20, 31, 0): (235, 31),
    (20, 20, 33, 0): (235, 33),
    (20, 20, 47, 0): (235, 47),
    (20, 20, 49, 0): (235, 49),
}
# ... and N on and around the streamed halves' 16-row edges, 40 items to draw from (D is what N rows
# reach: D <= min(N, 40))
N_EDGES = {
    (4, 8, 40, 11): (15, 12),
    (4, 8, 40, 1): (16, 14),
    (4, 8, 40, 14): (17, 14),
    (8, 8, 40, 10): (33, 22),
    (8, 8, 40, 87): (47, 29),
    (8, 8, 40, 52): (49, 31),
    (20, 12, 40, 1): (129, 39),
}
TINY = {(3, 6, 12, 0): (13, 8)}  # N < 16 and D < 16: one half of one block in both directions


def _run(gpu, monkeypatch, p, what):
    monkeypatch.setattr(ops, "_NCE_FUSED_ROWGRAD", True)
    paths.check(p, paths.run_grouped(gpu, p, "f16"), what)


@pytest.mark.parametrize("shape,nd", list(D_EDGES.items()) + list(N_EDGES.items()) + list(TINY.items()),
                         ids=lambda v: "-".join(map(str, v)))
def test_f16_block_edges(gpu, monkeypatch, shape, nd):
    p = paths.problem(*shape)
    assert (p["n"], p["d"]) == nd
    _run(gpu, monkeypatch, p, f"edge {shape}")


def _problem_from(users, t, W, lq, U, tau):
    """paths.problem's dictionary and float64 reference for given rows (N <= 1024: one chunk)."""
    n = users.numel()
    uniq = torch.unique(t)
    U64 = U.double().requires_grad_()
    W64 = W.double().requires_grad_()
    rows, _ = _nce_rows_ref(U64, W64[t], lq[t].double(), t, t, users, users, tau, 6, 0)
    loss = rows.sum() / n
    loss.backward()
    return dict(users=users, t=t, W=W, lq=lq, U=U, uniq=uniq, n=n, d=uniq.numel(), loss=loss.item(), dU=U64.grad,
                dW=W64.grad[uniq], row_loss=rows.detach())


def _hand_built():
    """70 rows over items 1..40 (all present: column = item - 1), seven users of ten rows, except that
    user 1 holds rows 10..21 and user 2 rows 22..29:
      - user 1's rows straddle the 16-row edge inside the first tile (rows 10..15 | 16..21);
      - its targets are items 4 and 20, columns 3 and 19 = 3 + 16: the same lane of both owner halves of
        wave 0, and item 30 (column 29);
      - items 4 and 20 also occur under other users (weight c - n > 0 on user 1's rows), item 30 only
        under user 1 (weight 0: the forward's -inf logit and the column pass's clamp)."""
    lens = [10, 12, 8, 10, 10, 10, 10]
    users = torch.repeat_interleave(torch.arange(7), torch.tensor(lens))
    t = torch.empty(70, dtype=torch.long)
    t[10:22] = torch.tensor([4, 20, 30, 4, 20, 4, 20, 30, 20, 4, 4, 20])
    rest = [r for r in range(70) if not 10 <= r < 22]
    others = [it for it in range(1, 41) if it != 30]  # 39 items, each at least once, 4 and 20 among them
    for k, r in enumerate(rest):
        t[r] = others[k % len(others)]
    g = torch.Generator().manual_seed(21)
    W = F.normalize(torch.randn(41, 128, generator=g), dim=1)
    lq = torch.log_softmax(torch.randn(41, generator=g), 0)
    U = F.normalize(torch.randn(70, 128, generator=g), dim=1)
    return users, t, W, lq, U


_CACHE = {}


def test_f16_user_across_halves_and_single_user_column(gpu, monkeypatch):
    if "hand" not in _CACHE:
        _CACHE["hand"] = _problem_from(*_hand_built(), paths.TAU)
    p = _CACHE["hand"]
    users, t = p["users"], p["t"]
    assert p["d"] == 40 and torch.equal(p["uniq"], torch.arange(1, 41))
    u1 = (users == 1).nonzero().flatten()
    assert u1.min() == 10 and u1.max() == 21  # rows on both sides of row 16 of tile 0
    cols = set((t[u1] - 1).tolist())
    assert {3, 19} <= cols  # columns c and c + 16 of wave 0
    assert set(users[t == 30].tolist()) == {1} and (t == 30).sum() == 2  # one user holds every instance
    assert set(users[t == 4].tolist()) > {1} and set(users[t == 20].tolist()) > {1}
    _run(gpu, monkeypatch, p, "hand-built")


def _near_converged(tau):
    """Rows = their label's item vector plus small noise (0.01 per component, as in tests/
    test_gpu_fullsize.py::test_grouped_logq_loss_near_converged), zero logQ, N ~ 300: the row gradient
    is a small difference of two near-equal vectors and the label pairs' column weights sit at the clamp.

    The item vectors share a common direction, pairwise cosine kappa = 0.36. With some 300 competing
    columns a row keeps 1 - p_pos ~ 300 exp(-(1 - kappa) / tau) ~ 3e-2 of its mass off its label, the
    regime of the full-size test (p_pos > 0.9), which at N ~ 300 isotropic items cannot reach: there
    p_pos = 0.9996, and the criterion is below what fp32 logits resolve. A logit of 1 / tau ~ 14.3 has
    an fp32 ulp of 2^-20, so p_pos - 1 carries an absolute error near 1e-6 whatever the kernel, and a
    gradient proportional to it is good to 1e-3 of its scale only while 1 - p_pos is well above 1e-3."""
    g = torch.Generator().manual_seed(31)
    lens = torch.randint(1, 21, (30,), generator=g)
    users = torch.repeat_interleave(torch.arange(30), lens)
    n = users.numel()
    t = torch.randint(1, 121, (n,), generator=g)
    kappa = 0.36
    c = F.normalize(torch.randn(128, generator=g), dim=0)
    W = F.normalize(kappa ** 0.5 * c + (1 - kappa) ** 0.5 * F.normalize(torch.randn(121, 128, generator=g), dim=1),
                    dim=1)
    U = F.normalize(W[t] + 0.01 * torch.randn(n, 128, generator=g), dim=1)
    return _problem_from(users, t, W, torch.zeros(121), U, tau)


def test_f16_near_converged(gpu, monkeypatch):
    """The label pairs' column weights p - 1 ~ -0.05 are small differences here: the column pass must
    round them to fp16 once, at their own magnitude (a common weight plus a separately rounded
    correction leaves 3e-4 per label row, 9e-3 of this batch's max|dW|)."""
    tau = 0.07
    monkeypatch.setattr(paths, "TAU", tau)  # run_grouped's temperature
    if "near" not in _CACHE:
        _CACHE["near"] = _near_converged(tau)
    p = _CACHE["near"]
    assert 250 <= p["n"] <= 350, p["n"]
    p_pos = torch.exp(-p["row_loss"])  # each row's softmax mass on its own label
    assert 0.9 < float(p_pos.median()) < 0.99 and float(p_pos.min()) > 0.85, (float(p_pos.median()), float(p_pos.min()))
    _run(gpu, monkeypatch, p, "near-converged")


_GP2_CHILD = """
import sys, torch
sys.path.insert(0, {root!r})
import recsys_amd
from recsys_amd import _native, ops
from tests import test_gpu_nce_paths as paths
_native.load()
ops._NCE_FUSED_ROWGRAD = True
gpu = torch.device("cuda:0")
for shape in [(20, 20, 17, 0), (8, 8, 40, 52)]:
    p = paths.problem(*shape)
    paths.check(p, paths.run_grouped(gpu, p, "f16"), "GP=2 %s" % (shape,))
print("gp2 ok")
"""


def test_f16_two_gradient_products(gpu):
    """RSX_NCE_F16_GP=2 (gradient products on the rows' hi and lo images) is read once per process, at
    the first f16 launch: a fresh child with the variable set runs two of the edge shapes."""
    env = dict(os.environ, RSX_NCE_F16_GP="2")
    r = subprocess.run([sys.executable, "-c", _GP2_CHILD.format(root=ROOT)], cwd=ROOT, env=env, capture_output=True,
                       text=True, timeout=300)
    print(r.stdout)
    assert r.returncode == 0 and "gp2 ok" in r.stdout, r.stdout + r.stderr
