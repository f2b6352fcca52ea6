"""Every kernel form of the DeepFM rerank forward against float64, at the edges of its row blocking, field
chunking and table variants, driven through the C ABI (csrc/deepfm_fused.hip, csrc/deepfm.hip):

  deepfm_fused_k   F in [1, 24] or [49, 64]     64 rows per workgroup, fields in chunks of 13
  deepfm_persist_k F in [25, 48] except 39      64 rows per iteration, one workgroup per CU looping over row
                                                blocks, fields in chunks of 8; packed or raw tables
  deepfm_rows5_k   F = 39, packed == NULL       128 rows per workgroup (four 32-row waves + a W1 stager)
  deepfm_rows2m_k  F = 39, packed tables        256 rows per workgroup (eight 32-row waves)
  unfused          rsx_deepfm_embed + rsx_linear_fwd + rsx_linear_dot_fwd (what training runs)

Inputs, reference and tolerance: tests/deepfm_fwd_ref.py (float64 oracle; |logit - ref| <= TOL = 1e-4 on
every row, rtol 0; tests/test_deepfm_fwd_ref_cpu.py shows that this bound at this input scale rejects a
kernel that drops one lo image of a bf16x3 product). prob: |prob - sigmoid(ref)| <= 0.25 TOL + 2e-7 (0.25:
sigmoid's Lipschitz constant; 2e-7: fp32 rounding of a value <= 1).

Canaries in every run: logit and prob sit between 64-float margins of a sentinel, the workspace and every
packed table are followed by 4 KiB of sentinel; all must be bit-unchanged (the kernels re-read the last row
for their tail lanes and must never store them). Packed runs get V / W arrays of decoy tables filled with a
large constant: the packed forms read the packed tables and nothing else. No test here provokes a fault:
every id is in range and every buffer is sized as include/recsys_amd.h says."""
import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import _native as N
from tests import deepfm_fwd_ref as D
from tests.deepfm_fwd_ref import TOL

pytestmark = pytest.mark.gpu

PROB_TOL = 0.25 * TOL + 2e-7
LIN_TOL = 2e-6           # x (1 + |ref|): rsx_deepfm_embed's fp32 bias + first order + FM
SENT = -12345.0          # float sentinel (NaN-free)
MARGIN = 64              # sentinel floats on each side of logit / prob
PAD = 4096               # sentinel bytes after the workspace and after each packed table
PAD_BYTE = 0xA5
DECOY = 1.0e3
R_MAX = 600
SEED = 1


def w_null(F, w):
    """Fields without a first-order table in variant w."""
    return {"given": (), "null": tuple(range(F)), "ends": (0, F - 1)}[w]


def canaried(n, dev):
    buf = torch.full((n + 2 * MARGIN,), SENT, device=dev, dtype=torch.float32)
    return buf, buf[MARGIN:MARGIN + n]


def margins_intact(buf, n):
    want = torch.full((MARGIN,), SENT).view(torch.int32)
    got = buf.cpu().view(torch.int32)
    return torch.equal(got[:MARGIN], want) and torch.equal(got[MARGIN + n:], want)


class DevCase:
    """A case of deepfm_fwd_ref on the device: tables, decoys, DNN, the prepared workspace, packed tables and
    float64 references per first-order variant (each built once, never modified)."""

    def __init__(self, c, dev):
        self.c, self.dev, self.F = c, dev, c["F"]
        lib = N.lib()
        self.V = [t.to(dev) for t in c["V"]]
        self.W = [t.to(dev) for t in c["W"]]
        self.decoy_V = [torch.full_like(t, DECOY) for t in self.V]
        self.decoy_W = [torch.full_like(t, DECOY) for t in self.W]
        self.w1, self.b1, self.w2, self.b2, self.wo = (c[k].to(dev).contiguous() for k in ("w1", "b1", "w2", "b2", "wo"))
        self.ws_bytes = lib.rsx_deepfm_fused_workspace_bytes(self.F)
        assert self.ws_bytes > 0
        self.ws = torch.full((self.ws_bytes + PAD,), PAD_BYTE, device=dev, dtype=torch.uint8)
        N.check(lib.rsx_deepfm_fused_prep(self.F, N.ptr(self.w1), N.ptr(self.w2), N.ptr(self.ws), N.stream()), "prep")
        torch.cuda.synchronize()
        self.check_ws("prep")
        self._packed, self._ref, self._lin = {}, {}, {}

    def check_ws(self, what):
        tail = self.ws[self.ws_bytes:].cpu()
        assert (tail == PAD_BYTE).all(), f"F={self.F}: {what} wrote past rsx_deepfm_fused_workspace_bytes"

    def w_array(self, w):
        if w == "null":
            return None
        skip = w_null(self.F, w)
        return N.ptr_array([None if f in skip else t for f, t in enumerate(self.W)])

    def packed(self, w):
        """Packed tables built from W (w = "given") or from W == NULL (w = "null"), sentinel after each."""
        if w not in self._packed:
            out = []
            for f, v in enumerate(self.V):
                n = v.shape[0] * 32
                p = torch.full((n + PAD // 4,), SENT, device=self.dev, dtype=torch.float32)
                N.check(N.lib().rsx_deepfm_pack(N.ptr(v), N.ptr(self.W[f]) if w == "given" else None, v.shape[0],
                                                N.ptr(p), N.stream()), "pack")
                out.append(p)
            torch.cuda.synchronize()
            self._packed[w] = out
            self.check_packed(w)
            for f, p in enumerate(out):  # the layout the header documents
                img = p[:-PAD // 4].view(-1, 32).cpu()
                assert torch.equal(img[:, :16], self.c["V"][f])
                assert torch.equal(img[:, 16], self.c["W"][f] if w == "given" else torch.zeros_like(self.c["W"][f]))
                assert (img[:, 17:] == 0).all()
        return self._packed[w]

    def check_packed(self, w):
        want = torch.full((PAD // 4,), SENT).view(torch.int32)
        for f, p in enumerate(self._packed[w]):
            assert torch.equal(p[-PAD // 4:].cpu().view(torch.int32), want), f"F={self.F}: field {f}'s packed tail written"

    def x_for(self, R):
        """The case's first R rows, the last of them again every field's last id."""
        x = self.c["x"][:R].clone()
        if R > 2:
            x[R - 1] = self.c["last"]
        return x

    def _fix(self, full, R):
        out = full[:R].clone()
        if R > 2:
            out[R - 1] = full[1]  # row 1 is every field's last id
        return out

    def ref(self, R, w="given"):
        if w not in self._ref:
            self._ref[w] = D.reference(self.c, w_null=w_null(self.F, w))[0]
        return self._fix(self._ref[w], R)

    def lin_ref(self, R, w="given"):
        if w not in self._lin:
            self._lin[w] = D.lin_reference(self.c, w_null=w_null(self.F, w))
        return self._fix(self._lin[w], R)


@pytest.fixture(scope="module")
def cases(gpu):
    """(F) -> DevCase at R_MAX rows, built once per module."""
    built = {}

    def get(F, R=R_MAX):
        if (F, R) not in built:
            built[(F, R)] = DevCase(D.make_case(F, R, SEED), gpu)
        return built[(F, R)]
    return get


@pytest.fixture(scope="module", autouse=True)
def worst():
    """Worst figures per form, printed once at the end of the module."""
    w = {}
    yield w
    print("\nDeepFM forward forms, worst figures:")
    for k in sorted(w):
        print(f"  {k}: {w[k]:.3e}")


def note(worst, key, val):
    worst[key] = max(worst.get(key, 0.0), val)


def run(dc, x, w="given", packed=None, with_prob=True, oneshot=False):
    """rsx_deepfm_fused_run (or the one-shot rsx_deepfm_fused) on rows x with the canaries checked.
    packed: None (raw tables, first-order variant w) or "given" / "null" (packed tables; V / W are decoys).
    Returns (logit, prob or None) on the CPU."""
    lib, F, R = N.lib(), dc.F, x.shape[0]
    xd = x.to(dc.dev)
    lbuf, logit = canaried(R, dc.dev)
    pbuf, prob = canaried(R, dc.dev)
    if packed is not None:
        tables = dc.packed(packed)
        Vp, Wp, Pp = N.ptr_array(dc.decoy_V), N.ptr_array(dc.decoy_W), N.ptr_array(tables)
    else:
        Vp, Wp, Pp = N.ptr_array(dc.V), dc.w_array(w), None
    pp = N.ptr(prob) if with_prob else None
    if oneshot:
        assert packed is None
        rc = lib.rsx_deepfm_fused(N.ptr(xd), R, F, Vp, Wp, dc.c["bias"], N.ptr(dc.w1), N.ptr(dc.b1), N.ptr(dc.w2),
                                  N.ptr(dc.b2), N.ptr(dc.wo), N.ptr(dc.ws), N.ptr(logit), pp, N.stream())
    else:
        rc = lib.rsx_deepfm_fused_run(N.ptr(xd), R, F, Vp, Wp, Pp, dc.c["bias"], N.ptr(dc.b1), N.ptr(dc.b2),
                                      N.ptr(dc.wo), N.ptr(dc.ws), N.ptr(logit), pp, N.stream())
    N.check(rc, "deepfm_fused_run")
    torch.cuda.synchronize()
    assert margins_intact(lbuf, R), f"F={F} R={R}: logit written outside [0, R)"
    assert margins_intact(pbuf, R), f"F={F} R={R}: prob written outside [0, R)"
    dc.check_ws("run")
    if packed is not None:
        dc.check_packed(packed)
    if not with_prob:
        assert (pbuf.cpu() == SENT).all()
        return logit.cpu(), None
    return logit.cpu(), prob.cpu()


def compare(worst, form, what, logit, prob, ref):
    err = (logit.double() - ref).abs().max().item()
    perr = (prob.double() - torch.sigmoid(ref)).abs().max().item()
    pself = (prob.double() - torch.sigmoid(logit.double())).abs().max().item()  # the sigmoid's own fp32 error
    print(f"  {form} {what}: logit err {err:.3e} prob err {perr:.3e} (to sigmoid of its own logit {pself:.3e})")
    note(worst, f"{form} logit", err)
    note(worst, "prob (all forms)", perr)
    note(worst, "prob to sigmoid of its own logit (reported only)", pself)
    assert torch.isfinite(logit).all() and err <= TOL, (form, what, err)
    assert perr <= PROB_TOL, (form, what, perr)


def sweep(cases, worst, form, F, Rs, w="given", packed=None):
    dc = cases(F)
    ref_w = packed if packed is not None else w
    print()
    for R in Rs:
        logit, prob = run(dc, dc.x_for(R), w=w, packed=packed)
        compare(worst, form, f"F={F} R={R} W {w} packed {packed}", logit, prob, dc.ref(R, ref_w))


# ---- the matrix ---------------------------------------------------------------------------------------------
def test_dispatch_is_the_documented_table(gpu):
    for F in range(1, 65):
        assert N.lib().rsx_deepfm_fused_uses_packed(F) == (1 if 25 <= F <= 48 else 0), F


# F = 1: one field; 13 / 14: one full chunk / a second chunk of one field; 24: a second chunk of 11;
# 49: a fourth chunk of 10; 64: the largest F (a fifth chunk of 12)
@pytest.mark.parametrize("w", ["given", "null"])
@pytest.mark.parametrize("F", [1, 13, 14, 24, 49, 64])
def test_fused_k(cases, worst, F, w):
    sweep(cases, worst, "deepfm_fused_k", F, (1, 63, 64, 65, 200), w=w)


def test_fused_k_per_field_null(cases, worst):
    sweep(cases, worst, "deepfm_fused_k", 14, (1, 65), w="ends")


# F = 25: the smallest F of the schedule (four chunks, the last of one field; odd: id_stride = F);
# 40: five full chunks (id_stride = F + 1); 48: the largest (six full chunks, every id-load slot used)
@pytest.mark.parametrize("variant", ["packed", "raw", "raw-null", "raw-ends", "packed-null"])
@pytest.mark.parametrize("F", [25, 40, 48])
def test_persist_k(cases, worst, F, variant):
    w, packed = {"packed": ("given", "given"), "raw": ("given", None), "raw-null": ("null", None),
                 "raw-ends": ("ends", None), "packed-null": ("null", "null")}[variant]
    sweep(cases, worst, "deepfm_persist_k", F, (1, 63, 64, 65, 200), w=w, packed=packed)


# R = 1 / 31 / 32 / 33: one wave partial, full, a second wave with one row and two waves with no row at
# all (they still keep the barrier count); 127 / 128 / 129 / 300: a second and a third workgroup
@pytest.mark.parametrize("w", ["given", "null", "ends"])
def test_rows5_k(cases, worst, w):
    sweep(cases, worst, "deepfm_rows5_k", 39, (1, 31, 32, 33, 127, 128, 129, 300), w=w)


def test_rows5_k_one_shot(cases, worst):
    dc = cases(39)
    x = dc.x_for(129)
    logit, prob = run(dc, x, oneshot=True)
    print()
    compare(worst, "deepfm_rows5_k", "F=39 R=129 rsx_deepfm_fused", logit, prob, dc.ref(129))
    again, _ = run(dc, x)
    assert torch.equal(logit, again)  # prep + run is the one-shot call


@pytest.mark.parametrize("w", ["given", "null"])
def test_rows2m_k(cases, worst, w):
    sweep(cases, worst, "deepfm_rows2m_k", 39, (1, 32, 33, 255, 256, 257, 600), w=w, packed=w)


def unfused(dc, x, w="given", with_emb=True):
    """The three-kernel path with every output canaried: (emb or None, lin, logit, prob) on the CPU."""
    lib, F, R, dev = N.lib(), dc.F, x.shape[0], dc.dev
    xd = x.to(dev)
    ebuf, emb = canaried(R * F * 16, dev)
    bufs = [canaried(R, dev) for _ in range(3)]
    (nbuf, lin), (lbuf, logit), (pbuf, prob) = bufs
    h1 = torch.empty(R, D.H1, device=dev, dtype=torch.float32)
    N.check(lib.rsx_deepfm_embed(N.ptr(xd), R, F, 16, N.ptr_array(dc.V), dc.w_array(w), dc.c["bias"],
                                 N.ptr(emb) if with_emb else None, N.ptr(lin), N.stream()), "embed")
    if with_emb:
        N.check(lib.rsx_linear_fwd(N.ptr(emb), F * 16, N.ptr(dc.w1), N.ptr(dc.b1), R, D.H1, F * 16, 1, N.ptr(h1),
                                   N.stream()), "linear")
        N.check(lib.rsx_linear_dot_fwd(N.ptr(h1), D.H1, N.ptr(dc.w2), N.ptr(dc.b2), R, D.H2, D.H1, 1, N.ptr(dc.wo),
                                       N.ptr(lin), N.ptr(logit), N.ptr(prob), N.stream()), "linear_dot")
    torch.cuda.synchronize()
    assert margins_intact(ebuf, R * F * 16) and all(margins_intact(b, R) for b, _ in bufs)
    if not with_emb:
        assert (ebuf.cpu() == SENT).all()
        return None, lin.cpu(), None, None
    return emb.cpu().view(R, F * 16), lin.cpu(), logit.cpu(), prob.cpu()


@pytest.mark.parametrize("w", ["given", "null"])
@pytest.mark.parametrize("F", [1, 39, 64])
def test_unfused(cases, worst, F, w):
    dc = cases(F)
    print()
    for R in (1, 65, 300):
        x = dc.x_for(R)
        emb, lin, logit, prob = unfused(dc, x, w=w)
        assert torch.equal(emb, torch.cat([dc.c["V"][f][x[:, f]] for f in range(F)], dim=1))
        lref = dc.lin_ref(R, w)
        lerr = ((lin.double() - lref).abs() / (1 + lref.abs())).max().item()
        print(f"  unfused F={F} R={R} W {w}: lin_out err / (1 + |ref|) {lerr:.3e}")
        note(worst, "unfused lin_out / (1 + |ref|)", lerr)
        assert lerr <= LIN_TOL, lerr
        compare(worst, "unfused", f"F={F} R={R} W {w}", logit, prob, dc.ref(R, w))


def test_unfused_without_emb_out(cases):
    dc = cases(39)
    x = dc.x_for(65)
    _, lin, _, _ = unfused(dc, x)
    _, lin_only, _, _ = unfused(dc, x, with_emb=False)
    assert torch.equal(lin, lin_only)


# ---- the persistent loop: second and third iterations, ids[it & 1] reused, a partial last block -----------
# F = 48 and 40 (six and five chunks) issue chunks of block `it` after block it + 1's ids are loaded, so they
# depend on the two id buffers: a build that kept one buffer was off by 6.6 and 4.8 here and passed every
# one-iteration test. F = 25 (four chunks) has issued all of a block's chunks by then; it covers the
# register-set rotation across blocks (4 chunks against 3 sets) and the odd id stride.
@pytest.mark.parametrize("F,packed", [(25, "given"), (48, "given"), (40, None)])
def test_persist_k_loops(gpu, worst, F, packed):
    cus = torch.cuda.get_device_properties(gpu).multi_processor_count
    R = (2 * cus + 37) * 64 - 13  # 37 workgroups make three iterations, the rest two
    dc = DevCase(D.make_case(F, R, SEED), gpu)
    x = dc.c["x"]
    ref = D.reference(dc.c)[0]
    logit, prob = run(dc, x, packed=packed)
    print()
    key = f"deepfm_persist_k long F={F} {'packed' if packed else 'raw'}"
    compare(worst, key, f"R={R} ({cus} CUs)", logit, prob, ref)
    again, pagain = run(dc, x, packed=packed)
    assert torch.equal(logit, again) and torch.equal(prob, pagain)
    # one block per workgroup on the same workgroups: any difference comes from the loop
    first, pfirst = run(dc, x[:64 * cus], packed=packed)
    diff = (logit[:64 * cus] != first).nonzero().flatten()
    assert diff.numel() == 0, f"rows {diff[:8].tolist()}.. of {diff.numel()} differ from the one-iteration run"
    assert torch.equal(prob[:64 * cus], pfirst)


# ---- prob == NULL, determinism, R = 0: once per form ----------------------------------------------------
FORMS = [("deepfm_fused_k", 13, None, 200), ("deepfm_persist_k", 40, "given", 200), ("deepfm_persist_k", 25, None, 200),
         ("deepfm_rows5_k", 39, None, 300), ("deepfm_rows2m_k", 39, "given", 600)]


@pytest.mark.parametrize("form,F,packed,R", FORMS)
def test_prob_null_and_determinism(cases, form, F, packed, R):
    dc = cases(F)
    x = dc.x_for(R)
    logit, prob = run(dc, x, packed=packed)
    again, pagain = run(dc, x, packed=packed)
    assert torch.equal(logit, again) and torch.equal(prob, pagain)
    alone, _ = run(dc, x, packed=packed, with_prob=False)
    assert torch.equal(logit, alone)


def test_unfused_prob_null_and_determinism(cases):
    dc = cases(39)
    x = dc.x_for(300)
    _, lin, logit, prob = unfused(dc, x)
    _, lin2, logit2, prob2 = unfused(dc, x)
    assert torch.equal(lin, lin2) and torch.equal(logit, logit2) and torch.equal(prob, prob2)
    h1 = torch.randn(300, D.H1, device=dc.dev)
    outs = []
    for with_prob in (True, False):
        lbuf, lg = canaried(300, dc.dev)
        pbuf, pr = canaried(300, dc.dev)
        N.check(N.lib().rsx_linear_dot_fwd(N.ptr(h1), D.H1, N.ptr(dc.w2), N.ptr(dc.b2), 300, D.H2, D.H1, 1, N.ptr(dc.wo),
                                           None, N.ptr(lg), N.ptr(pr) if with_prob else None, N.stream()), "linear_dot")
        torch.cuda.synchronize()
        assert margins_intact(lbuf, 300) and margins_intact(pbuf, 300)
        if not with_prob:
            assert (pbuf.cpu() == SENT).all()
        outs.append(lg.cpu())
    assert torch.equal(outs[0], outs[1])


@pytest.mark.parametrize("form,F,packed,R", FORMS)
def test_zero_rows(cases, form, F, packed, R):
    dc = cases(F)
    xd = dc.x_for(1).to(dc.dev)
    lbuf, logit = canaried(8, dc.dev)
    pbuf, prob = canaried(8, dc.dev)
    Pp = N.ptr_array(dc.packed(packed)) if packed else None
    rc = N.lib().rsx_deepfm_fused_run(N.ptr(xd), 0, F, N.ptr_array(dc.V), N.ptr_array(dc.W), Pp, dc.c["bias"],
                                      N.ptr(dc.b1), N.ptr(dc.b2), N.ptr(dc.wo), N.ptr(dc.ws), N.ptr(logit), N.ptr(prob),
                                      N.stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert (lbuf.cpu() == SENT).all() and (pbuf.cpu() == SENT).all()
    dc.check_ws("run with R = 0")
