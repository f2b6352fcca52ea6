"""Every kernel form of the token GEMM (csrc/gemm_x3.hip) against float64, at its tile edges.

The dispatcher is a product of forms: the weight-stationary kernel gemm_ws_k<KC, NBW, EPI> (K 128 / 256 /
384, B as stored or transposed, seven epilogues), the LDS-staged stream gemm_x3_nt_k<EPI, Q, BK> (two stages;
four stages in flight at 32 or at 16 of K per stage) and split-K with the epilogue in gemm_splitk_reduce_k.
Each case first asserts rsx_gemm_x3_form (and the split count), the function gemm_x3_impl itself switches on,
so a retuned dispatcher that moves a shape to another form fails here instead of silently leaving a form
untested. The C ABI is called directly: leading dimensions, a null workspace and a null bias are the test's.

Operands of every case are strided (lda = K + 8, ldb = K + 12, ldbt = N + 4, ldc = N + 4, ldaux = N + 8; the
pads of A / B / aux-in hold NaN). C and aux have one row more than M and are filled with a sentinel: the pad
columns and the extra row must hold it bit for bit afterwards (the weight-stationary kernel stores float4s
and rewrites row M - 1 from its tail lanes).

Comparisons (tests/gemm_forms_ref.py holds operands and restatements):
  (a) integer operands: the product is exact in fp32, so the kernel equals the fp32 restatement of the
      epilogue over the float64 product bit for bit (for a linear epilogue that is float64 itself);
  (b) the three lo probes, exact too, whose expected value is the documented three-term sum;
      GELU outputs of (a) / (b) are held to gemm_forms_ref.gelu_exact_bound (the function's own error);
  (c) N(0, 1) operands, per element: |C - f64| <= 2e-5 sum|a||b| + 1e-6 (times the keep scale; GELU outputs
      by the propagated bounds 1.13 bnd / (1 - p) + 2e-6 and 0.6 bnd + 2e-6 of tests/test_gpu_kernels.py);
  (d) N(0, 1) operands, per tensor, tests/test_gpu_glue.py's rule with the fp32 emulation of the bf16x3
      product as the restatement: max|kernel - f64| <= 8 max|emulation - f64| + 8 * 2^-24 max|f64|.
      The 0 / 1 mask that the training ReLU saves is not a rounding quantity: it must equal (z > 0) wherever
      |z| exceeds the bound of (c).
Dropout forms also run at p = 0: the zeroed set equals the host mask over m * N + n (N, not ldc), kept
elements equal the p = 0 result times scale32(p) bit for bit, and aux does not depend on p.
Add + LayerNorm: s is a GEMM output as above; y, mean and rstd are compared by rule (d) with LayerNorm of
the kernel's own s in float64 and in fp32, so an error of the LayerNorm cannot hide inside the GEMM's bound.
That comparison runs on the integer and the N(0, 1) operands, whose rows have |mean| <~ std. The lo probes
are operands for the product, not for a LayerNorm: rows of the two-sided probe sit at K +- 8, |mean| / std ~
100, where one ulp of the row sum (3e-5 of the mean at K = 256) is the whole error and only the order of the
fp32 summation decides it. There the kernel (64 sequential adds per lane, one exchange) measured 2.455e-05
on y at 129 x 128 x 256 against 1.882e-06 for torch's blocked fp32 sum, over the rule's 1.807e-05, with mean
off by 1.2 ulp; s of those cases is still compared exactly.

Largest kernel / emulation ratio of rule (d) seen per form (pytest -s prints them):
  two-stage 1.04, four-stage BK 32 1.04, four-stage BK 16 1.02, split-K 1.04, weight-stationary 1.05 (GEMM
  outputs and GELU's aux; the bf16x3 kernels and the emulation differ in summation order only);
  weight-stationary add+LN: s 1.02; y 5.94, mean 4.00, rstd 5.06 over the edge shapes and 4.66 over the
  65,569-row strip-loop case, M = 1 aside. The single row of 1 x 128 x 256 (integers) reads 47.43 and 8.75 on
  rstd and is no miss of the rule: the fp32 restatement happens to land within 4.0e-11 and 1.9e-10 of float64
  there, while the kernel's 1.9e-09 and 1.7e-09 are a quarter ulp of rstd and sit under the rule's
  8 * 2^-24 * max|f64| term (bounds 9.95e-09 and 1.12e-08). The factor stays 8 for every form.
"""
import functools
import math

import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import _native as N
from tests import gemm_forms_ref as R

pytestmark = pytest.mark.gpu

F32, F64 = torch.float32, torch.float64
_U = 2.0 ** -24
SENT = -12345.678          # what C / aux hold before the call
P_DROP = 0.3               # scale32(0.3) is not a power of two: a misplaced multiply shows
EPS = 1e-5
_RATIO = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    for form in sorted(_RATIO):
        print(f"\n  largest kernel / emulation ratio, {form}: {_RATIO[form]:.2f}", end="")
    print()


# ------------------------------------------------------------------------------------ comparison rules
def _cmp(form, name, got, f64, f32):
    """tests/test_gpu_glue.py's rule for one tensor: kernel result, float64 reference, fp32 restatement."""
    assert got.dtype == F32 and f64.dtype == F64 and f32.dtype == F32, name
    assert tuple(got.shape) == tuple(f64.shape), (name, tuple(got.shape), tuple(f64.shape))
    assert torch.isfinite(got).all(), name
    ek = (got.double() - f64).abs().max().item()
    er = (f32.double() - f64).abs().max().item()
    bound = 8.0 * er + 8.0 * _U * f64.abs().max().item()
    ratio = ek / er if er > 0 else (0.0 if ek == 0 else math.inf)
    if math.isfinite(ratio):
        _RATIO[form] = max(_RATIO.get(form, 0.0), ratio)
    print(f"  {name}: kernel {ek:.3e}  fp32 {er:.3e}  ratio {ratio:.2f}  bound {bound:.3e}")
    assert ek <= bound, f"{name}: kernel error {ek:.3e} > bound {bound:.3e} (fp32 restatement {er:.3e})"


def _exact(name, got, want):
    assert got.dtype == want.dtype and tuple(got.shape) == tuple(want.shape), (name, got.dtype, tuple(got.shape))
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{name}: {bad.shape[0]} of {got.numel()} elements differ, first at {list(i)}: "
                             f"{got[i].item()!r} != {want[i].item()!r}")


def _within(name, got, ref64, bound):
    err = (got.double() - ref64).abs()
    bad = err > bound
    if bad.any():
        i = tuple(bad.nonzero()[0].tolist())
        raise AssertionError(f"{name}: {int(bad.sum())} elements over the bound, first at {list(i)}: error "
                             f"{err[i].item():.3e} > {bound[i].item():.3e}")


# ------------------------------------------------------------------------------------ buffers and calls
def _padded(t, ld, dev, rows=None):
    """t [r, c] as the leading block of a [rows, ld] device buffer whose other elements are NaN."""
    buf = torch.full((rows or t.shape[0], ld), float("nan"))
    buf[: t.shape[0], : t.shape[1]] = t
    return buf.to(dev)


class _Out:
    """An output [M, n] inside a sentinel-filled [M + 1, ld] device buffer."""

    def __init__(self, M, n, ld, dev):
        self.M, self.n = M, n
        self.buf = torch.full((M + 1, ld), SENT, device=dev) if ld else torch.full((M + 1,), SENT, device=dev)

    def take(self, name):
        host = self.buf.cpu()
        sent = torch.tensor(SENT)
        if host.dim() == 1:
            assert host[self.M] == sent, f"{name}: the element past M was written"
            return host[: self.M].clone()
        assert bool((host[self.M] == sent).all()), f"{name}: the row past M was written"
        assert bool((host[: self.M, self.n:] == sent).all()), f"{name}: pad columns were written"
        return host[: self.M, : self.n].clone()


def _run(gpu, entry, kind, a, w, bias, p=0.0, aux_in=None, with_ws=True, want_aux=True, table=None, ridx=None,
         x=None, ln=None):
    """One call of the C ABI on strided operands; {name: host tensor} of every output, pads checked."""
    lib = N.lib()
    M, K = a.shape
    n = w.shape[0]
    lda, ldb, ldc, ldaux = K + 8, K + 12, n + 4, n + 8
    A = _padded(a, lda, gpu)
    B = _padded(w.T.contiguous(), n + 4, gpu) if entry == "tn" else _padded(w, ldb, gpu)
    bias_d = None if bias is None else bias.to(gpu)
    C = _Out(M, n, ldc, gpu)
    outs = {"C": C}
    aux_ptr = None
    if kind == "dgelu":
        aux_d = _padded(aux_in, ldaux, gpu)
        aux_ptr = aux_d.data_ptr()
    elif kind in ("gelu", "relu_train") and want_aux:
        outs["aux"] = _Out(M, n, ldaux, gpu)
        aux_ptr = outs["aux"].buf.data_ptr()
    st = N.stream()
    if entry == "nt":
        floats = lib.rsx_gemm_x3_split_floats(M, n, K) if with_ws else 0
        ws = torch.empty(floats, device=gpu) if floats else None
        if kind == "relu_train":
            rc = lib.rsx_gemm_x3_relu_train(A.data_ptr(), lda, B.data_ptr(), ldb, N.ptr(bias_d), M, n, K, aux_ptr,
                                            ldaux, p, R.SEED, C.buf.data_ptr(), ldc, N.ptr(ws), floats, st)
        elif with_ws:
            rc = lib.rsx_gemm_x3_ws(A.data_ptr(), lda, B.data_ptr(), ldb, N.ptr(bias_d), M, n, K, R.EPI[kind],
                                    aux_ptr, ldaux, p, R.SEED, C.buf.data_ptr(), ldc, N.ptr(ws), floats, st)
        else:
            rc = lib.rsx_gemm_x3(A.data_ptr(), lda, B.data_ptr(), ldb, N.ptr(bias_d), M, n, K, R.EPI[kind],
                                 aux_ptr, ldaux, p, R.SEED, C.buf.data_ptr(), ldc, st)
    elif entry == "tn":
        rc = lib.rsx_gemm_x3_tn(A.data_ptr(), lda, B.data_ptr(), n + 4, N.ptr(bias_d), M, n, K, R.EPI[kind],
                                aux_ptr, ldaux, p, R.SEED, C.buf.data_ptr(), ldc, st)
    elif entry == "rowadd":
        T = _padded(table, ldaux, gpu)
        ridx_d = ridx.to(gpu)
        rc = lib.rsx_gemm_x3_rowadd(A.data_ptr(), lda, B.data_ptr(), ldb, N.ptr(bias_d), M, n, K, T.data_ptr(),
                                    ldaux, ridx_d.data_ptr(), C.buf.data_ptr(), ldc, st)
    else:
        X = _padded(x, ldaux, gpu)
        lw, lb = ln[0].to(gpu), ln[1].to(gpu)
        outs.update(y=_Out(M, n, ldc, gpu), mean=_Out(M, 1, 0, gpu), rstd=_Out(M, 1, 0, gpu))
        rc = lib.rsx_gemm_x3_addln(A.data_ptr(), lda, B.data_ptr(), ldb, N.ptr(bias_d), M, n, K, X.data_ptr(),
                                   ldaux, p, R.SEED, lw.data_ptr(), lb.data_ptr(), EPS, C.buf.data_ptr(), ldc,
                                   outs["y"].buf.data_ptr(), ldc, outs["mean"].buf.data_ptr(),
                                   outs["rstd"].buf.data_ptr(), st)
    N.check(rc, f"{entry} {kind} {M}x{n}x{K}")
    torch.cuda.synchronize()
    return {k: o.take(f"{entry} {kind} {M}x{n}x{K} {k}") for k, o in outs.items()}


# ------------------------------------------------------------------------------------ shared references
@functools.lru_cache(maxsize=12)
def _exact_set(which, M, n, K):
    """(a, w, bias, acc): acc = the exact three-term product, kept as fp32 (it is representable)."""
    seed = 7919 * M + 31 * n + K + {"int": 0, "a": 1, "b": 2, "ab": 3}[which]
    if which == "int":
        a, w, b = R.int_case(M, n, K, seed)
        acc = a.double() @ w.double().T
    else:
        a, w, b, z = R.probe_case(which, M, n, K, seed)
        acc = z - b.double()
    acc32 = acc.float()
    assert torch.equal(acc32.double(), acc)
    return a, w, b, acc32


@functools.lru_cache(maxsize=4)
def _float_set(M, n, K):
    a, w, b = R.float_case(M, n, K, seed=104729 * M + 17 * n + K)
    return a, w, b, a.double() @ w.double().T, R.emulate32(a, w), 2e-5 * R.absprod(a, w)


def _side_inputs(kind, entry, M, n, exact, seed):
    """The epilogue's own operands: dgelu's aux, rowadd's table and row indices, addln's residual."""
    g = torch.Generator().manual_seed(seed)
    kw = {}
    if kind == "dgelu":
        if exact:
            vals = torch.tensor([-2.0, -1.0, -0.5, 0.5, 1.0, 1.5])
            kw["aux"] = vals[torch.randint(0, 6, (M, n), generator=g)]
        else:
            kw["aux"] = R.gelu_grad(torch.randn(M, n, generator=g))
    if entry == "rowadd":
        rows = 7
        kw["table"] = (torch.randint(-4, 4, (rows, n), generator=g).float() + 0.5 if exact
                       else torch.randn(rows, n, generator=g))
        ridx = torch.randint(0, rows, (M,), generator=g)
        ridx[0] = rows - 1                   # the last table row, and repeats
        ridx[M - 1] = ridx[0]
        kw["ridx"] = ridx
    if entry == "addln":
        kw["x"] = (torch.randint(-4, 4, (M, n), generator=g).float() + 0.5 if exact
                   else torch.randn(M, n, generator=g))
    return kw


def _check_ln(form, tag, out, ln):
    s = out["C"]
    y64, m64, r64 = R.layer_norm(s.double(), ln[0], ln[1], EPS)
    y32, m32, r32 = R.layer_norm(s, ln[0], ln[1], EPS)
    _cmp(form, f"{tag} y", out["y"], y64, y32)
    _cmp(form, f"{tag} mean", out["mean"], m64, m32)
    _cmp(form, f"{tag} rstd", out["rstd"], r64, r32)


def _case(gpu, form, entry, kind, M, n, K, with_ws=True, want_aux=True, p_drop=P_DROP, floats_too=True):
    """All comparisons of one (entry, epilogue, shape)."""
    ekind = "rowadd" if entry == "rowadd" else "addln" if entry == "addln" else kind
    drops = ekind in ("gelu", "dgelu", "relu_train", "addln")
    p = p_drop if drops else 0.0
    ln = None
    if entry == "addln":
        g = torch.Generator().manual_seed(M + K)
        ln = (1.0 + 0.5 * torch.randn(n, generator=g), torch.randn(n, generator=g))
    tag0 = f"{form} {entry} {ekind} {M}x{n}x{K}"

    # (a), (b): exact operands, at the dropout rate; integers once more without a bias
    for which, bias_on in (("int", True), ("a", True), ("b", True), ("ab", True), ("int", False)):
        if not bias_on and ekind == "dgelu":
            continue
        a, w, b, acc = _exact_set(which, M, n, K)
        b = b if bias_on else None
        side = _side_inputs(ekind, entry, M, n, True, seed=M * n + K)
        out = _run(gpu, entry, ekind, a, w, b, p, side.get("aux"), with_ws, want_aux, side.get("table"),
                   side.get("ridx"), side.get("x"), ln)
        tag = f"{tag0} {which}{'' if bias_on else ' no bias'}"
        c32, x32 = R.epilogue(ekind, acc, F32, bias=b, p=p, **side)
        if ekind == "gelu":
            c64, x64 = R.epilogue(ekind, acc, F64, bias=b, p=p, **side)
            _within(f"{tag} C", out["C"], c64, R.gelu_exact_bound(c64, p))
            assert not out["C"][~R.keep_mask(R.SEED, p, M, n)].any(), f"{tag}: a dropped element is not 0"
            if want_aux:
                _within(f"{tag} aux", out["aux"], x64, R.gelu_exact_bound(x64))
        else:
            _exact(f"{tag} C", out["C"], c32)
            if ekind == "relu_train":
                _exact(f"{tag} aux", out["aux"], x32)
        if entry == "addln" and which == "int":
            _check_ln(form, tag, out, ln)
    if not floats_too:
        return

    # (c), (d): N(0, 1) operands at p = 0 and, for the dropout forms, at p
    a, w, b, acc64, emu, bnd = _float_set(M, n, K)
    side = _side_inputs(ekind, entry, M, n, False, seed=M * n + K + 1)
    res = {}
    for pp in sorted({0.0, p}):
        out = res[pp] = _run(gpu, entry, ekind, a, w, b, pp, side.get("aux"), with_ws, want_aux, side.get("table"),
                             side.get("ridx"), side.get("x"), ln)
        tag = f"{tag0} randn p={pp}"
        c64, x64 = R.epilogue(ekind, acc64, F64, bias=b, p=pp, **side)
        c32, x32 = R.epilogue(ekind, emu, F32, bias=b, p=pp, **side)
        sc = R.scale_of(pp, F64).item()
        if ekind == "gelu":
            _within(f"{tag} C", out["C"], c64, 1.13 * bnd * sc + 2e-6)
            if want_aux:
                _within(f"{tag} aux", out["aux"], x64, 0.6 * bnd + 2e-6)
                _cmp(form, f"{tag} aux", out["aux"], x64, x32)
        elif ekind == "dgelu":
            _within(f"{tag} C", out["C"], c64, bnd * sc * side["aux"].double().abs() + 1e-6)
        else:
            _within(f"{tag} C", out["C"], c64, (bnd + 1e-6) * sc)
        _cmp(form, f"{tag} C", out["C"], c64, c32)
        if ekind == "relu_train":
            z64 = acc64 + b.double()
            sure = z64.abs() > bnd + 1e-6
            assert sure.double().mean() > 0.99
            _exact(f"{tag} aux", out["aux"][sure], x64.float()[sure])
            assert bool(((out["aux"] == 0) | (out["aux"] == 1)).all()), tag
        if entry == "addln":
            _check_ln(form, tag, out, ln)
    if p > 0 and entry != "addln":
        c0, cp = res[0.0]["C"], res[p]["C"]
        keep = R.keep_mask(R.SEED, p, M, n)
        live = c0 != 0
        assert live.double().mean() > 0.3 or M * n < 1000, tag0     # gelu(z) underflows for z < -13
        assert torch.equal((cp == 0)[live], (~keep)[live]), f"{tag0}: zeroed set != host mask over m * N + n"
        _exact(f"{tag0} kept = p0 * scale32", cp, torch.where(keep, c0 * R.scale_of(p, F32), torch.zeros(())))
        if "aux" in res[p]:
            _exact(f"{tag0} aux(p) == aux(0)", res[p]["aux"], res[0.0]["aux"])


def _assert_form(M, n, K, kind, with_ws, form, S):
    lib = N.lib()
    floats = lib.rsx_gemm_x3_split_floats(M, n, K)
    got = lib.rsx_gemm_x3_form(M, n, K, R.EPI[kind], floats if with_ws else 0)
    assert got == form, f"{M}x{n}x{K} {kind}: form {got}, the table says {form}"
    if form == R.FORM_SPLIT:
        assert floats == S * M * n, (M, n, K, floats, S)


def _table(group, K, kind):
    rows = [r for r in R.form_table() if r[0] == group and r[3] == K and r[4] == kind]
    assert rows
    return rows


def _need_256_cus():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert cus == 256, f"the form table is written for 256 CUs, this device has {cus}"


# ------------------------------------------------------------------------------------ the streamed forms
@pytest.mark.parametrize("kind", R.STREAM_EPIS)
@pytest.mark.parametrize("K", [16, 32, 48, 96])
def test_two_stage_short_k(gpu, K, kind):
    """gemm_x3_nt_k<EPI>: 1, 2, 3 and 6 stages (the has_next edges of the two-stage loop), M around the
    128-row tile and past two tiles, one and two column tiles."""
    _need_256_cus()
    for _, M, n, _, _, ws, form, S in _table("two", K, kind):
        _assert_form(M, n, K, kind, ws, form, S)
        _case(gpu, "two-stage", "nt", kind, M, n, K, ws)


def test_two_stage_at_least_cus_tiles(gpu):
    """2049 x 2048 x 512: 17 x 16 = 272 tiles >= 256 CUs, so neither split-K nor the four-stage form; the
    last row block holds one row. Integers, probes and floats on the bias epilogue."""
    _need_256_cus()
    (_, M, n, K, kind, ws, form, S), = [r for r in R.form_table() if r[0] == "two_big"]
    _assert_form(M, n, K, kind, ws, form, S)
    _case(gpu, "two-stage", "nt", kind, M, n, K, ws)


@pytest.mark.parametrize("kind", R.STREAM_EPIS)
@pytest.mark.parametrize("K", [288, 320, 352, 544, 512])
def test_four_stage_bk32(gpu, K, kind):
    """gemm_x3_nt_k<EPI, 4, 32>: 9, 10, 11, 17 and (K = 512 through the entry without a workspace) 16 stages,
    every residue mod 4 of how the in-flight loop ends. The dGELU epilogue keeps the two-stage kernel at these
    shapes and must report form 1."""
    _need_256_cus()
    for _, M, n, _, _, ws, form, S in _table("four32", K, kind):
        _assert_form(M, n, K, kind, ws, form, S)
        _case(gpu, "two-stage" if kind == "dgelu" else "four-stage BK 32", "nt", kind, M, n, K, ws)


@pytest.mark.parametrize("kind", ["bias", "gelu"])
@pytest.mark.parametrize("K", [272, 304])
def test_four_stage_bk16(gpu, K, kind):
    """gemm_x3_nt_k<EPI, 4> at 16 of K per stage (K % 32 == 16): 17 and 19 stages."""
    _need_256_cus()
    for _, M, n, _, _, ws, form, S in _table("four16", K, kind):
        _assert_form(M, n, K, kind, ws, form, S)
        _case(gpu, "four-stage BK 16", "nt", kind, M, n, K, ws)


@pytest.mark.parametrize("kind", R.STREAM_EPIS)
@pytest.mark.parametrize("K", [512, 768, 1024, 2048])
def test_split_k(gpu, K, kind):
    """S = 2, 3, 4, 8 K-ranges of 256 per tile, the epilogue in gemm_splitk_reduce_k<EPI> (all five)."""
    _need_256_cus()
    for _, M, n, _, _, ws, form, S in _table("split", K, kind):
        _assert_form(M, n, K, kind, ws, form, S)
        _case(gpu, "split-K", "nt", kind, M, n, K, ws)


# ------------------------------------------------------------------------------------ weight-stationary
WS_M = (1, 31, 32, 33, 127, 129)


@pytest.mark.parametrize("kind", R.WS_NT_EPIS)
@pytest.mark.parametrize("K", [128, 256, 384])
def test_weight_stationary_edges_nt(gpu, K, kind):
    """gemm_ws_k<KC, NBW, EPI>, B as stored: one strip and less, two strips, the 128-row round and one row
    past it; one and three column blocks (six at K = 384)."""
    noaux = kind == "gelu_noaux"
    kind = "gelu" if noaux else kind
    for _, M, n, _, _, ws, form, S in _table("ws", K, kind):
        _assert_form(M, n, K, kind, ws, form, S)
        _case(gpu, "weight-stationary", "nt", kind, M, n, K, ws, want_aux=not noaux)


@pytest.mark.parametrize("kind", ["bias", "gelu", "dgelu"])
@pytest.mark.parametrize("K", [128, 256, 384])
def test_weight_stationary_edges_tn(gpu, K, kind):
    """The same with B transposed (rsx_gemm_x3_tn, ldbt = N + 4)."""
    for n in (128, 384):
        for M in WS_M:
            _case(gpu, "weight-stationary", "tn", kind, M, n, K)


@pytest.mark.parametrize("K", [128, 256])
def test_weight_stationary_rowadd(gpu, K):
    """rsx_gemm_x3_rowadd: ridx with repeats and the last table row."""
    for n in (128, 384):
        for M in WS_M:
            _case(gpu, "weight-stationary", "rowadd", "rowadd", M, n, K)


@pytest.mark.parametrize("p", [0.0, 0.2])
@pytest.mark.parametrize("K", [128, 256])
def test_weight_stationary_addln(gpu, K, p):
    """rsx_gemm_x3_addln: s as a GEMM output, y / mean / rstd against LayerNorm of the kernel's own s."""
    for M in WS_M:
        _case(gpu, "weight-stationary add+LN", "addln", "addln", M, 128, K, p_drop=p)


STRIP = [("nt", "bias", 1024, 128), ("nt", "relu_train", 1024, 128), ("tn", "bias", 1024, 128),
         ("rowadd", "rowadd", 1024, 128),
         ("nt", "bias", 1024, 256), ("nt", "relu_train", 1024, 256), ("tn", "bias", 1024, 256),
         ("rowadd", "rowadd", 1024, 256),
         ("nt", "bias", 1024, 384), ("nt", "relu_train", 1024, 384), ("tn", "bias", 1024, 384),
         ("addln", "addln", 128, 128), ("addln", "addln", 128, 256)]


@pytest.mark.parametrize("entry,kind,n,K", STRIP)
def test_weight_stationary_strip_loop(gpu, entry, kind, n, K):
    """M = 2 * 128 * (CUs / nblk) + 33 with the device's CU count: some waves own three 32-row strips, the
    rest two, so the double-buffered load / compute loop iterates, ends on odd and on even item counts
    (nmine * KC), clamps its trailing prefetches and resets the accumulators between strips. Integers and
    probes only (exact)."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    M = R.strip_rows(cus, n, K)
    groups = max(cus // (n // (64 if K == 384 else 128)), 1)
    strips = (M + 31) // 32
    assert 2 * 4 * groups < strips < 3 * 4 * groups          # every wave owns two or three strips
    if entry == "nt":
        _assert_form(M, n, K, kind, True, R.FORM_WS, 0)
    _case(gpu, "weight-stationary add+LN" if entry == "addln" else "weight-stationary", entry, kind, M, n, K,
          p_drop=0.2 if entry == "addln" else P_DROP, floats_too=False)
