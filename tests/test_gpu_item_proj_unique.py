"""item_proj once per distinct item: the device step index hands the tower the pretrained rows of the
batch's Uq distinct items plus each token's slot among them (ops.ItemRows) instead of one row per token
of each view. item_proj (rsx_gemm_x3) runs over the Uq rows, rsx_seq_embed_fwd / _bwd read its output
through the slots (base_idx), and item_proj's weight gradient comes from the per-item sums of the
embedding stage's per-token input gradient.

A GEMM output row depends only on its own input row and the weights, so the tower's output and every
gradient except item_proj's own are bit-identical to the per-token form ("fallback": the same batch with
the rows materialised per token); item_proj's dW / db change in summation order only and are held
against a float64 per-token product."""
import math

import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import _native as N
from recsys_amd import dist as D
from recsys_amd import ops, synth
from recsys_amd.tower_code import v1_refine_usertower as T
from tests.helpers import small_cfg, small_universe, to_dev

pytestmark = pytest.mark.gpu

_L, _DM = 50, 128


# ---------------------------------------------------------------------------------------------------
# indexed base of the embedding kernels
def _embed_inputs(gpu, n_live):
    """1003 packed tokens (no multiple of 32, more than one workgroup of the forward), ids of table 0
    drawn from 37 values including the padding id 0; base holds one row per distinct id."""
    g = torch.Generator().manual_seed(7)
    t = 1003
    rows = [501, 40, 51, 51, 51, 51]
    ids = [torch.randint(0, 37, (t,), generator=g)] + [torch.randint(0, r, (t,), generator=g) for r in rows[1:]]
    ids[0][:5] = 0
    tables = [torch.randn(r, _DM, generator=g) * 0.5 for r in rows]
    gate = torch.zeros(6)
    gate[:n_live] = torch.rand(n_live, generator=g) + 0.25
    pos = torch.randn(_L, _DM, generator=g) * 0.5
    tok_pos = torch.randint(0, _L, (t,), generator=g)
    ln_w, ln_b = torch.rand(_DM, generator=g) + 0.5, torch.randn(_DM, generator=g) * 0.1
    dout = torch.randn(t, _DM, generator=g)
    dev = lambda x: x.to(gpu)
    ids = [dev(i) for i in ids]
    seg = ops.sort_segments(ids[0])
    uniq = seg[4]
    slot = torch.full((int(uniq.max()) + 1,), -1, dtype=torch.int64, device=gpu)
    slot[uniq] = torch.arange(uniq.numel(), device=gpu)
    base_idx = slot[ids[0]]
    base_u = dev(torch.randn(uniq.numel(), _DM, generator=g))
    return dict(ids=ids, tables=[dev(x) for x in tables], gate=dev(gate), pos=dev(pos), tok_pos=dev(tok_pos),
                ln_w=dev(ln_w), ln_b=dev(ln_b), dout=dev(dout), seg=seg, base_idx=base_idx, base_u=base_u)


def _embed_native(a, base, base_idx, p, seed):
    """rsx_seq_embed_fwd / _bwd called directly: (out, mean, rstd, per-token dbase, dgate, dpos)."""
    lib = N.lib()
    t = a["ids"][0].numel()
    out = torch.empty(t, _DM, device=base.device)
    mean, rstd = torch.empty(t, device=base.device), torch.empty(t, device=base.device)
    rc = lib.rsx_seq_embed_fwd(N.ptr(base), N.ptr(base_idx), N.ptr_array(a["ids"]), N.ptr_array(a["tables"]), 6,
                               N.ptr(a["gate"]), N.ptr(a["pos"]), N.ptr(a["tok_pos"]), N.ptr(a["ln_w"]),
                               N.ptr(a["ln_b"]), 1e-5, t, _L, _DM, p, seed, N.ptr(out), N.ptr(mean), N.ptr(rstd),
                               N.stream())
    N.check(rc, "seq_embed_fwd")
    dbase = torch.empty(t, _DM, device=base.device)
    # no table gradients here: the larger tables' scatter-adds are atomic (their last bits vary run to run)
    dgate, dpos = torch.zeros_like(a["gate"]), torch.zeros_like(a["pos"])
    dlw, dlb = torch.zeros_like(a["ln_w"]), torch.zeros_like(a["ln_w"])
    nws = lib.rsx_seq_embed_bwd_workspace_floats(t, _L, _DM)
    ws = torch.empty(nws, device=base.device)
    rc = lib.rsx_seq_embed_bwd(N.ptr(base), N.ptr(base_idx), N.ptr_array(a["ids"]), N.ptr_array(a["tables"]),
                               N.i64_array([x.shape[0] for x in a["tables"]]), N.i64_array([0] * 6), 6,
                               N.ptr(a["gate"]), N.ptr(a["pos"]), N.ptr(a["tok_pos"]), N.ptr(a["ln_w"]), N.ptr(mean),
                               N.ptr(rstd), 1e-5, t, _L, _DM, p, seed, N.ptr(a["dout"]), N.ptr(dbase),
                               N.ptr_array([None] * 6), N.ptr(dgate), N.ptr(dpos), N.ptr(dlw), N.ptr(dlb),
                               N.ptr(ws), nws, N.stream())
    N.check(rc, "seq_embed_bwd")
    torch.cuda.synchronize()
    return out, mean, rstd, dbase, dgate, dpos, dlw, dlb


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("n_live", [1, 2, 6])
def test_seq_embed_indexed_base_equals_materialised(gpu, p, n_live):
    """base[base_idx[t]] read by the kernels equals the same call on the materialised rows, bit for bit:
    output, saved statistics, the per-token dbase and every sum the backward forms. n_live picks the
    kernel form: 2 live tables is the packed tower's compile-time configuration, 6 the generic
    one-row-at-a-time form, 1 the run-time-tested grouped form."""
    a = _embed_inputs(gpu, n_live)
    assert a["ids"][0].numel() % 32 != 0 and int((a["ids"][0] == 0).sum()) >= 5
    seed = 0x5EED if p > 0 else 0
    got = _embed_native(a, a["base_u"], a["base_idx"], p, seed)
    ref = _embed_native(a, a["base_u"][a["base_idx"]].contiguous(), None, p, seed)
    for k, (x, y) in enumerate(zip(got, ref)):
        assert torch.equal(x, y), k
    assert got[3].shape == (a["ids"][0].numel(), _DM)          # dbase stays per token


@pytest.mark.parametrize("p", [0.0, 0.2])
def test_seq_embed_op_indexed_base(gpu, p):
    """ops.seq_embed(base_idx=...): the output equals the call on base[base_idx] bit for bit (same torch
    seed, hence the same dropout seed); base's gradient [Uq, 128] is the per-slot sum of the materialised
    call's per-token gradient, held against its float64 sum within n * 2^-24 * sum|terms| per element
    (n = the slot's tokens: the bound of an fp32 sum of n terms in any order); the gate's and table 0's
    gradients are bit-identical (formed from the same per-token values by the same deterministic sums;
    the time table's scatter-add is atomic and not compared)."""
    a = _embed_inputs(gpu, 2)
    res = []
    for indexed in (True, False):
        base = (a["base_u"] if indexed else a["base_u"][a["base_idx"]]).clone().requires_grad_()
        tabs = [x.clone().requires_grad_() for x in a["tables"]]
        gate = a["gate"].clone().requires_grad_()
        torch.manual_seed(3)
        out = ops.seq_embed(base, a["ids"], tabs, gate, a["pos"], a["ln_w"], a["ln_b"], p_drop=p,
                            padding_idx=[0] * 6, tok_pos=a["tok_pos"], tab0_seg=a["seg"],
                            base_idx=a["base_idx"] if indexed else None)
        out.backward(a["dout"])
        torch.cuda.synchronize()
        res.append((out.detach(), base.grad, [x.grad for x in tabs], gate.grad))
    (o1, b1, t1, g1), (o2, b2, t2, g2) = res
    assert torch.equal(o1, o2) and torch.equal(g1, g2) and torch.equal(t1[0], t2[0])
    assert b1.shape == a["base_u"].shape and b2.shape == o2.shape
    idx = a["base_idx"]
    ref = torch.zeros_like(b1, dtype=torch.float64).index_add_(0, idx, b2.double())
    mag = torch.zeros_like(ref).index_add_(0, idx, b2.double().abs())
    n = torch.bincount(idx, minlength=b1.shape[0]).double().unsqueeze(1)
    assert ((b1.double() - ref).abs() <= n * 2.0 ** -24 * mag).all()


# ---------------------------------------------------------------------------------------------------
# the tower: distinct-item form against the per-token form on the same batch
def _batch(gpu, case):
    """96 users x 50 (as tests/test_gpu_tower.py) with the catalogue's ids, or 8 users with a degenerate
    id set: one item for every token; every token of a view a different item; 37 items (below one
    128-row GEMM tile, no multiple of 32)."""
    items = small_universe(500)
    b = 96 if case == "catalogue" else 8
    batch = synth.make_batch(items, b, seed=21)
    n = b * _L
    if case == "one_item":
        batch["item_ids"] = torch.full((b, _L), 7, dtype=batch["item_ids"].dtype)
    elif case == "all_distinct":
        batch["item_ids"] = (torch.arange(n) + 1).reshape(b, _L).to(batch["item_ids"].dtype)
    elif case == "uq37":
        batch["item_ids"] = (torch.arange(n) * 7 % 37).reshape(b, _L).to(batch["item_ids"].dtype)
    return to_dev(batch, gpu), items.pretrained.to(gpu)


def _run(gpu, ix, pv, p, native, tail, spy=False):
    """One forward + backward of forward_packed; returns (out, {parameter gradients}, pv.grad, dBase)."""
    pk, pk2, tok_ids, _, static = ix.packed
    torch.manual_seed(5)
    model = T.SASRecUserTower(small_cfg(num_items=500, dropout=p)).to(gpu).train()
    seen = []
    orig = ops.linear_tok

    def linear_tok(x, w, b=None):  # keeps the gradient of item_proj's output (the per-token dBase)
        y = orig(x, w, b)
        if w is model.item_proj.weight:
            y.retain_grad()
            seen.append(y)
        return y

    prev = ops._TOWER_NATIVE
    ops._TOWER_NATIVE = native
    if spy:
        ops.linear_tok = linear_tok
    try:
        assert (ops.tower_native_ok(model, pk2, pv) is not None) == native
        torch.manual_seed(9)
        out = model.forward_packed(pk2, pv, tok_ids, *static, tail_last=pk.last_tok if tail else None)
        w = torch.randn(out.shape, generator=torch.Generator().manual_seed(3)).to(gpu)
        (out * w).sum().backward()
    finally:
        ops._TOWER_NATIVE = prev
        ops.linear_tok = orig
    torch.cuda.synchronize()
    grads = {n: q.grad.detach().clone() for n, q in model.named_parameters() if q.grad is not None}
    dpv = pv.grad if torch.is_tensor(pv) and pv.requires_grad else None
    return out.detach(), grads, dpv, (seen[0].grad if seen else None)


_PROJ = ("item_proj.weight", "item_proj.bias")


def _same_but_proj(a, b):
    assert torch.equal(a[0], b[0])
    assert a[1].keys() == b[1].keys() and len(a[1]) > 40
    for n in a[1]:
        if n not in _PROJ:
            assert torch.equal(a[1][n], b[1][n]), n


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("case", ["catalogue", "one_item", "all_distinct", "uq37"])
def test_tower_per_item_against_per_token(gpu, case, p):
    """The tower from (pv_u, tok_uidx) against the per-token form of the same batch (the index's rows
    materialised: what both paths run without the distinct-item plan or with a pretrained-row gradient).

    Output and every gradient except item_proj's: torch.equal, on the per-op path, the native program and
    its tail form; the native program and the per-op path agree bit for bit on item_proj's too (same
    entry points, same arguments). item_proj dW / db: against float64 dBase^T pretrained[ids] and
    sum_t dBase over the per-token dBase (the gradient of item_proj's output in the per-token per-op
    run), within tests/test_gpu_kernels.py::test_linear_wgrad_against_float64's bf16x3 bound:
    |dW - ref| <= 2e-5 (|dBase|^T |x| + sqrt(T)) per element, |db - ref| <= 2e-5 sqrt(T)."""
    batch, lookup = _batch(gpu, case)
    ix = D.prepare_step_index(batch, pretrained_lookup=lookup)
    pv = ix.packed[3]
    assert isinstance(pv, ops.ItemRows)
    uq, t2 = pv.rows.shape[0], pv.idx.numel()
    if case == "one_item":
        assert uq == 1
    elif case == "all_distinct":
        assert 2 * uq == t2
    elif case == "uq37":
        assert uq < 128 and uq % 32 != 0 and uq > 1
    tok = pv.materialize()
    assert tok.shape == (t2, _DM) and torch.equal(tok, lookup[ix.packed[2][0]])
    n_mat = ops.ItemRows.materialized
    item = _run(gpu, ix, pv, p, native=True, tail=False)
    item_ops = _run(gpu, ix, pv, p, native=False, tail=False)
    assert ops.ItemRows.materialized == n_mat                   # neither path fell back to the [T, 128] rows
    tok_ops = _run(gpu, ix, tok, p, native=False, tail=False, spy=True)
    tok_nat = _run(gpu, ix, tok, p, native=True, tail=False)
    # the native program and the per-op path, distinct-item form: everything bit-identical
    assert torch.equal(item[0], item_ops[0])
    for n in item[1]:
        assert torch.equal(item[1][n], item_ops[1][n]), n
    # distinct-item form against the per-token form
    _same_but_proj(item, tok_ops)
    _same_but_proj(item, tok_nat)
    _same_but_proj(_run(gpu, ix, pv, p, native=True, tail=True), _run(gpu, ix, tok, p, native=True, tail=True))
    dbase = tok_ops[3].double().cpu()
    x = tok.double().cpu()
    assert dbase.shape == (t2, _DM)
    ref_w, ref_b = dbase.t() @ x, dbase.sum(0)
    s = 2e-5 * math.sqrt(t2)
    for r in (item, tok_nat):     # the distinct-item form, and the per-token form under the same bound
        ew = (r[1][_PROJ[0]].double().cpu() - ref_w).abs()
        eb = (r[1][_PROJ[1]].double().cpu() - ref_b).abs()
        assert (ew <= 2e-5 * (dbase.abs().t() @ x.abs()) + s).all()
        assert eb.max().item() <= s


def test_pretrained_gradient_takes_the_per_token_form(gpu):
    """A caller that asks for the pretrained rows' gradient passes them per token: the gradient comes back
    [T, 128], bit-identical between the native program and the per-op path (rsx_gemm_x3_tn over dBase),
    within the bf16x3 product bound of float64 dBase W (2e-5 |dBase| |W| + 1e-6 per element), and the
    output equals the distinct-item form's."""
    batch, lookup = _batch(gpu, "catalogue")
    ix = D.prepare_step_index(batch, pretrained_lookup=lookup)
    pv = ix.packed[3]
    res = []
    for native, spy in ((True, False), (False, True)):
        tok = pv.materialize().clone().requires_grad_()
        res.append(_run(gpu, ix, tok, 0.2, native=native, tail=False, spy=spy))
    (o1, g1, d1, _), (o2, g2, d2, dbase) = res
    assert d1.shape == (pv.idx.numel(), _DM) and torch.equal(d1, d2) and torch.equal(o1, o2)
    for n in g1:
        assert torch.equal(g1[n], g2[n]), n
    torch.manual_seed(5)
    w = T.SASRecUserTower(small_cfg(num_items=500, dropout=0.2)).item_proj.weight.detach().double()
    ref = dbase.double().cpu() @ w
    bound = 2e-5 * (dbase.double().cpu().abs() @ w.abs()) + 1e-6
    assert ((d1.double().cpu() - ref).abs() <= bound).all()
    assert torch.equal(o1, _run(gpu, ix, pv, 0.2, native=True, tail=False)[0])


def test_no_grad_forward_runs_the_per_item_form(gpu):
    """With gradients off forward_packed takes the per-op path; it keeps the distinct-item form (no
    [T, 128] rows materialised) and gives the training forward's output bit for bit (dropout 0)."""
    batch, lookup = _batch(gpu, "catalogue")
    ix = D.prepare_step_index(batch, pretrained_lookup=lookup)
    pk, pk2, tok_ids, pv, static = ix.packed
    ref = _run(gpu, ix, pv, 0.0, native=True, tail=False)[0]
    torch.manual_seed(5)
    model = T.SASRecUserTower(small_cfg(num_items=500, dropout=0.0)).to(gpu).train()
    n_mat = ops.ItemRows.materialized
    with torch.no_grad():
        out = model.forward_packed(pk2, pv, tok_ids, *static)
    assert ops.ItemRows.materialized == n_mat and torch.equal(out, ref)


def test_step_index_item_rows(gpu):
    """The index's distinct-item rows and slots: rows = lookup[uniq_items], uniq_items[slot[t]] = the
    token's item id for both views; the per-token view it stands for is materialised on demand."""
    batch, lookup = _batch(gpu, "catalogue")
    ix = D.prepare_step_index(batch, pretrained_lookup=lookup)
    pk, pk2, tok_ids, pv, _ = ix.packed
    uniq = pk2.item_seg[4]
    assert pv.rows.shape == (uniq.numel(), _DM) and pv.idx.dtype == torch.int64
    assert torch.equal(pv.rows, lookup[uniq])
    assert torch.equal(uniq[pv.idx], tok_ids[0])
    assert pv.shape == (2 * pk.flat.numel(), _DM) and pv.dtype == torch.float32 and pv.is_cuda
    assert torch.equal(pv, lookup[tok_ids[0]])
    assert len(pv) == tok_ids[0].numel() and torch.equal(pv[:3], lookup[tok_ids[0][:3]])
