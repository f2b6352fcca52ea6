"""Small-shape coverage of the contrastive-loss host dispatch (csrc/nce_plain.hip, nce_grouped.hip,
nce_grouped_f16.hip, nce_emphasis.hip): the shipped f16 / bf16x3 grouped paths with and without the
fused row gradient, every column-pass split order, the fused forward's partial-slot counts (both
regions of its tail geometry), accumulate != 0, and the atomic emphasis backward.

Reference: the float64 restatement _nce_rows_ref of tests/test_gpu_kernels.py on the CPU (the plain
N x N problem with same-item and same-user masks), evaluated in row chunks, once per shape.
Criteria, as tests/test_gpu_fullsize.py::test_grouped_logq_loss_full_size applies per precision:
mean loss within 1e-4, each gradient within 1e-3 of its reference's max-abs. Unit-norm rows,
tau = 0.1. Where two paths must agree exactly the comparison is torch.equal."""
import pytest
import torch
import torch.nn.functional as F

import recsys_amd  # noqa: F401
from recsys_amd import _native as N
from recsys_amd import ops
from tests.test_gpu_kernels import _nce_rows_ref

pytestmark = pytest.mark.gpu

TAU = 0.1
_PROBLEMS = {}


def problem(n_users, max_len, n_items, seed, need_dw=True):
    """A grouped LogQ problem on the CPU with its float64 reference (cached, never modified)."""
    key = (n_users, max_len, n_items, seed, need_dw)
    if key in _PROBLEMS:
        return _PROBLEMS[key]
    g = torch.Generator().manual_seed(seed)
    lens = torch.randint(1, max_len + 1, (n_users,), generator=g)
    users = torch.repeat_interleave(torch.arange(n_users), lens)
    n = users.numel()
    t = torch.randint(1, n_items + 1, (n,), generator=g)
    W = F.normalize(torch.randn(n_items + 1, 128, generator=g), dim=1)
    lq = torch.log_softmax(torch.randn(n_items + 1, generator=g), 0)
    U = F.normalize(torch.randn(n, 128, generator=g), dim=1)
    uniq = torch.unique(t)
    U64 = U.double().requires_grad_()
    W64 = W.double().requires_grad_(need_dw)
    total = 0.0
    for lo in range(0, n, 1024):  # row chunks: label of row i at column i (diag offset lo)
        hi = min(n, lo + 1024)
        rows, _ = _nce_rows_ref(U64[lo:hi], W64[t], lq[t].double(), t[lo:hi], t, users[lo:hi], users, TAU, 6, lo)
        part = rows.sum() / n
        part.backward()
        total += part.item()
    p = dict(users=users, t=t, W=W, lq=lq, U=U, uniq=uniq, n=n, d=uniq.numel(), loss=total, dU=U64.grad,
             dW=W64.grad[uniq] if need_dw else None)
    _PROBLEMS[key] = p
    return p


def run_grouped(gpu, p, precision):
    """(mean loss, dU, dW over the distinct targets) of ops.nce_grouped_sum as the step calls it."""
    Ud = p["U"].to(gpu).requires_grad_()
    grp = ops.TargetGroups(p["t"].to(gpu), p["users"].to(gpu))
    assert torch.equal(grp.uniq.cpu(), p["uniq"])
    items = p["W"].to(gpu)[grp.uniq].clone().requires_grad_()
    s, cnt = ops.nce_grouped_sum(Ud, items, p["lq"].to(gpu)[grp.uniq], grp, tau=TAU, precision=precision)
    assert int(cnt.item()) == p["n"]
    loss = s / cnt
    loss.backward()
    return loss.detach().cpu(), Ud.grad.cpu(), items.grad.cpu()


def check(p, out, what=""):
    loss, dU, dW = out
    print(f"{what} N={p['n']} D={p['d']} loss {loss.item():.7f} ref {p['loss']:.7f}", end="")
    grads = [("dU", dU, p["dU"])] + ([("dW", dW, p["dW"])] if p["dW"] is not None else [])
    errs = []
    for name, got, ref in grads:
        err, scale = (got.double() - ref).abs().max().item(), ref.abs().max().item()
        print(f" {name} err {err:.3e} scale {scale:.3e}", end="")
        errs.append((name, err, scale))
    print()
    assert abs(loss.item() - p["loss"]) < 1e-4, (loss.item(), p["loss"])
    for name, err, scale in errs:
        assert err <= 1e-3 * scale, (name, err, scale)


def col_splits(n, d):
    """The column pass's split count for bf16x3 / f16 (rsx_nce_grouped_bwd): 32 or 16 in the
    split-major order when they fit the 8 x max(N, D) partial rows and leave >= 2 tiles per split,
    else the plain order's 8 (4 when the distinct targets alone fill the chip)."""
    for want in (32, 16):
        if want * d <= 8 * max(n, d) and n >= want * 64:
            return want
    return 4 if -(-d // 128) * 4 >= 1024 else 8


# (n_users, max_len, n_items, seed), the column-pass splits the shape is meant to take
SHAPES = [
    ((7, 3, 5, 2), 8),          # fewer rows than one tile, D < 32
    ((40, 30, 25, 0), 8),       # D < 32: every tile an exception tile
    ((100, 30, 200, 3), 16),    # N in [1024, 2048), D <= N/2: 16-split split-major
    ((200, 30, 300, 4), 32),    # N >= 2048, D <= N/4: 32-split split-major
    ((300, 8, 20000, 5), 8),    # N >= 1024 but D > N/2: the plain 8-split order
]


def _shape_problem(shape, splits):
    p = problem(*shape)
    n, d = p["n"], p["d"]
    assert col_splits(n, d) == splits, (n, d)
    if shape[:3] == (7, 3, 5):
        assert n < 32 and d < 32
    elif shape[:3] == (40, 30, 25):
        assert d < 32 and n > 128
    elif splits == 16:
        assert 1024 <= n < 2048 and 2 * d <= n
    elif splits == 32:
        assert n >= 2048 and 4 * d <= n
    else:
        assert n >= 1024 and 2 * d > n
    return p


@pytest.mark.parametrize("precision", ["bf16x3", "f16"])
@pytest.mark.parametrize("shape,splits", SHAPES)
def test_grouped_fused_forward_and_column_pass(gpu, monkeypatch, shape, splits, precision):
    """rsx_nce_grouped_fwd_grad (loss + row gradient in one sweep) and the column pass of
    rsx_nce_grouped_bwd, at the shipped default and at bf16x3."""
    monkeypatch.setattr(ops, "_NCE_FUSED_ROWGRAD", True)
    p = _shape_problem(shape, splits)
    check(p, run_grouped(gpu, p, precision), f"fused {precision}")


@pytest.mark.parametrize("shape,splits", SHAPES)
def test_grouped_unfused_row_pass(gpu, monkeypatch, shape, splits):
    """rsx_nce_grouped_fwd plus the row pass of rsx_nce_grouped_bwd (nce_grouped_bwd_x3_k<true, false>).
    The f16 row pass re-splits B into bf16 images, so its row gradient (and the loss, which runs the
    bf16x3 logits) equals bf16x3's bit for bit."""
    monkeypatch.setattr(ops, "_NCE_FUSED_ROWGRAD", False)
    p = _shape_problem(shape, splits)
    x3 = run_grouped(gpu, p, "bf16x3")
    h = run_grouped(gpu, p, "f16")
    check(p, x3, "unfused bf16x3")
    check(p, h, "unfused f16")
    assert torch.equal(h[0], x3[0]) and torch.equal(h[1], x3[1])


def rb1(n, nsplit, cus):
    """Row blocks of the fused forward's first region (rsx_nce_grouped_fwd_grad): all of them, or for
    nsplit = 8 as many as fill whole rounds of 2 x CUs workgroups at 4 splits each."""
    rbs = -(-n // 128)
    if nsplit != 8:
        return rbs
    slots = 2 * cus
    return (4 * rbs // slots) * slots // 4


# N ~ 300, and N just above 128 x 128 rows with D <= 512 (row gradient only: the reference's dW is not needed)
NSPLIT_SIZES = {"small": ((20, 30, 80, 6), True), "tail": ((1090, 30, 400, 7), False)}


@pytest.mark.parametrize("precision", ["bf16x3", "f16"])
@pytest.mark.parametrize("nsplit", [1, 2, 4, 8])
@pytest.mark.parametrize("size", ["small", "tail"])
def test_grouped_fused_forward_partial_slots(gpu, monkeypatch, size, nsplit, precision):
    """The fused forward at every partial-slot count. At nsplit = 8 the tail geometry runs its first
    region only when 4 x row blocks fill a round of the grid: never at the small size, and at the other
    size both regions run (fwdg_geometry's two branches)."""
    monkeypatch.setattr(ops, "_NCE_FUSED_ROWGRAD", True)
    monkeypatch.setattr(ops, "_NSPLIT_FWD_GROUPED", nsplit)
    shape, need_dw = NSPLIT_SIZES[size]
    p = problem(*shape, need_dw=need_dw)
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    rbs = -(-p["n"] // 128)
    if size == "small":
        assert 200 <= p["n"] <= 400 and rb1(p["n"], 8, cus) == 0
    else:
        assert p["d"] <= 512 and 128 < rbs and 0 < rb1(p["n"], 8, cus) < rbs
    loss, dU, dW = run_grouped(gpu, p, precision)
    check(p, (loss, dU, dW), f"{size} nsplit {nsplit} {precision}")


# ---------------------------------------------------------------------------- accumulate != 0
def _unit(n, g):
    return F.normalize(torch.randn(n, 128, generator=g), dim=1)


def run_plain_accumulate(gpu, x3):
    """dA, dB of rsx_nce_bwd / rsx_nce_bwd_x3 into zeroed buffers (accumulate = 0), then again on top
    (accumulate = 1). N = 77, M = 300, same-item mask and bias."""
    n, m, flags = 77, 300, 2
    g = torch.Generator().manual_seed(11)
    A, B = _unit(n, g).to(gpu), _unit(m, g).to(gpu)
    bias = torch.log_softmax(torch.randn(m, generator=g), 0).to(gpu)
    k1b = torch.randint(0, 40, (m,), generator=g).to(torch.int32).to(gpu)
    k1a = k1b[:n].clone()
    lib = N.lib()
    nws = lib.rsx_nce_x3_workspace_floats(n, m) if x3 else lib.rsx_nce_workspace_floats(n, m, 8, 8)
    ws = torch.empty(nws, device=gpu)
    out2 = torch.empty(2, device=gpu)
    gout = torch.ones(1, device=gpu)
    head = (N.ptr(A), N.ptr(B), N.ptr(bias), N.ptr(k1a), N.ptr(k1b), None, None, n, m, 128, 128, 0, TAU, flags)
    if x3:
        N.check(lib.rsx_nce_fwd_x3(*head, N.ptr(ws), N.ptr(out2), N.stream()), "fwd_x3")
        bwd = lambda dA, dB, acc: lib.rsx_nce_bwd_x3(*head, N.ptr(gout), N.ptr(ws), N.ptr(dA), N.ptr(dB), acc, N.stream())
    else:
        N.check(lib.rsx_nce_fwd(*head, 8, N.ptr(ws), N.ptr(out2), N.stream()), "fwd")
        bwd = lambda dA, dB, acc: lib.rsx_nce_bwd(*head, 8, 8, N.ptr(gout), N.ptr(ws), N.ptr(dA), N.ptr(dB), acc,
                                                  N.stream())
    dA, dB = torch.zeros(n, 128, device=gpu), torch.zeros(m, 128, device=gpu)
    N.check(bwd(dA, dB, 0), "bwd")
    first = (dA.clone(), dB.clone())
    N.check(bwd(dA, dB, 1), "bwd accumulate")
    return out2.cpu(), first[0].cpu(), first[1].cpu(), dA.cpu(), dB.cpu()


def run_grouped_accumulate(gpu, precision):
    """The same through rsx_nce_grouped_fwd / rsx_nce_grouped_bwd: 77 rows of a 600-column batch with
    exactly 300 distinct targets (the sharded form of TargetGroups)."""
    g = torch.Generator().manual_seed(12)
    t_cols = torch.cat([torch.randperm(300, generator=g) + 1, torch.randint(1, 301, (300,), generator=g)])
    users = torch.repeat_interleave(torch.arange(60), 10)
    n = 77
    grp = ops.TargetGroups(t_cols[:n].to(gpu), users[:n].to(gpu), t_cols=t_cols.to(gpu))
    d = grp.n_cols
    assert d == 300
    A, B = _unit(n, g).to(gpu), _unit(d, g).to(gpu)
    bias = torch.log_softmax(torch.randn(d, generator=g), 0).to(gpu)
    prec = ops.NCE_PRECISIONS[precision]
    lib = N.lib()
    ws = torch.empty(lib.rsx_nce_grouped_workspace_floats(n, d, 2, 8, prec), device=gpu)
    out2 = torch.empty(2, device=gpu)
    gout = torch.ones(1, device=gpu)
    rows = (N.ptr(A), N.ptr(B), N.ptr(bias), N.ptr(grp.colcnt), N.ptr(grp.row_col), N.ptr(grp.row_beg),
            N.ptr(grp.row_end), N.ptr(grp.exc_cols))
    N.check(lib.rsx_nce_grouped_fwd(*rows, n, d, 128, 128, TAU, prec, 2, N.ptr(ws), N.ptr(out2), N.stream()), "fwd")
    cols = (N.ptr(grp.col_beg), N.ptr(grp.col_end), N.ptr(grp.exc_s), N.ptr(grp.exc_e), N.ptr(grp.exc_n))
    bwd = lambda dA, dB, acc: lib.rsx_nce_grouped_bwd(*rows, *cols, n, d, 128, 128, TAU, prec, 2, 8, N.ptr(gout),
                                                      N.ptr(ws), N.ptr(dA), N.ptr(dB), acc, N.stream())
    dA, dB = torch.zeros(n, 128, device=gpu), torch.zeros(d, 128, device=gpu)
    N.check(bwd(dA, dB, 0), "bwd")
    first = (dA.clone(), dB.clone())
    N.check(bwd(dA, dB, 1), "bwd accumulate")
    return out2.cpu(), first[0].cpu(), first[1].cpu(), dA.cpu(), dB.cpu()


def _check_accumulate(out):
    _, a1, b1, a2, b2 = out
    assert a1.abs().max() > 0 and b1.abs().max() > 0
    assert torch.equal(a2, a1 + a1) and torch.equal(b2, b1 + b1)  # x + x is exact in fp32


@pytest.mark.parametrize("x3", [False, True], ids=["fp32", "bf16x3"])
def test_plain_backward_accumulates(gpu, x3):
    _check_accumulate(run_plain_accumulate(gpu, x3))


@pytest.mark.parametrize("precision", ["fp32", "bf16x3", "f16"])
def test_grouped_backward_accumulates(gpu, precision):
    _check_accumulate(run_grouped_accumulate(gpu, precision))


# ---------------------------------------------------------------------------- emphasis backward
def run_emphasis(gpu, x3, n=300, K=1, N_rows=None):
    """dA, dB of rsx_nce_emphasis_bwd (atomic dB) and rsx_nce_emphasis_bwd_csr on top of `base`, after
    the dense flags-2 forward and rsx_nce_emphasis_fwd. Mined ids: a permutation (K = 1), so every
    column is mined once and the atomic form has one addend per element."""
    g = torch.Generator().manual_seed(13)
    A, B = _unit(n, g).to(gpu), _unit(n, g).to(gpu)
    bias = torch.log_softmax(torch.randn(n, generator=g), 0).to(gpu)
    k1 = torch.randint(0, 100, (n,), generator=g).to(torch.int32).to(gpu)
    top = torch.randperm(n, generator=g).view(n, 1).to(gpu)
    rows = n if N_rows is None else N_rows
    margin, prec = 0.5, 1 if x3 else 0
    lib = N.lib()
    nws = lib.rsx_nce_x3_workspace_floats(n, n) if x3 else lib.rsx_nce_workspace_floats(n, n, 8, 8)
    ws = torch.empty(nws, device=gpu)
    out2 = torch.empty(2, device=gpu)
    gout = torch.ones(1, device=gpu)
    head = (N.ptr(A), N.ptr(B), N.ptr(bias), N.ptr(k1), N.ptr(k1))
    dense = head + (None, None, n, n, 128, 128, 0, TAU, 2)
    if x3:
        N.check(lib.rsx_nce_fwd_x3(*dense, N.ptr(ws), N.ptr(out2), N.stream()), "fwd_x3")
    else:
        N.check(lib.rsx_nce_fwd(*dense, 8, N.ptr(ws), N.ptr(out2), N.stream()), "fwd")
    emph = head + (N.ptr(top), rows, n, K, 128, 128, 0, TAU, margin, prec, 8)
    if rows and K:
        N.check(lib.rsx_nce_emphasis_fwd(*emph, N.ptr(ws), N.ptr(out2), N.stream()), "emphasis_fwd")
    flat = top.reshape(-1)
    sk, col_ent = torch.sort(flat, stable=True)
    col_ptr = torch.searchsorted(sk, torch.arange(n + 1, device=gpu, dtype=sk.dtype)).contiguous()
    cbuf = torch.empty(n * max(K, 1), device=gpu)
    base = 0.0 if rows and K else 7.0  # the no-op calls must leave their targets alone
    dA1, dB1 = torch.full((n, 128), base, device=gpu), torch.full((n, 128), base, device=gpu)
    dA2, dB2 = dA1.clone(), dB1.clone()
    N.check(lib.rsx_nce_emphasis_bwd(*emph, N.ptr(gout), N.ptr(ws), N.ptr(dA1), N.ptr(dB1), N.stream()), "emphasis_bwd")
    N.check(lib.rsx_nce_emphasis_bwd_csr(*emph, N.ptr(col_ptr), N.ptr(col_ent), N.ptr(cbuf), N.ptr(gout), N.ptr(ws),
                                         N.ptr(dA2), N.ptr(dB2), N.stream()), "emphasis_bwd_csr")
    return out2.cpu(), dA1.cpu(), dB1.cpu(), dA2.cpu(), dB2.cpu()


@pytest.mark.parametrize("x3", [False, True], ids=["fp32", "bf16x3"])
def test_emphasis_backward_atomic_equals_csr(gpu, x3):
    _, dA1, dB1, dA2, dB2 = run_emphasis(gpu, x3)
    assert dA1.abs().max() > 0 and dB1.abs().max() > 0
    assert torch.equal(dA1, dA2) and torch.equal(dB1, dB2)


@pytest.mark.parametrize("K,rows", [(0, 300), (1, 0)], ids=["K0", "N0"])
def test_emphasis_backward_noops(gpu, K, rows):
    _, dA1, dB1, dA2, dB2 = run_emphasis(gpu, False, K=K, N_rows=rows)
    for t in (dA1, dB1, dA2, dB2):
        assert torch.equal(t, torch.full_like(t, 7.0))
