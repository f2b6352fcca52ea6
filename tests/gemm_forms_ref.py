"""Host references for the token GEMM's kernel forms (csrc/gemm_x3.hip): operands, float64 / fp32
restatements of every epilogue, an fp32 emulation of the bf16x3 product, and the table of shapes with the
form each must take (plain torch / numpy, no device).

Operands
  int_case     a in [-3, 3], w in [-2, 2], half-integer bias: hi = x and lo = 0 in the bf16 split, and every
               product and partial sum is an integer below 2^24 for K <= 3072, so the fp32 accumulation is
               exact in any order. A wrong row, column, k-slot, stride or tile edge changes the result.
  probe_case   exact as well, and sensitive to the lo fragments that integers leave at zero:
                 "a"   a = 1 + i/4096, i in [-7, 7] (hi = 1, lo = i/4096 exactly), b in {-1, 0, 1}
                 "b"   the mirror image: a in {-1, 0, 1}, b = 1 + j/4096
                 "ab"  both sides split. The kernel's documented product is hi*hi' + hi*lo' + lo*hi', so the
                       expected sum is sum_k (1 + (i + j)/4096), WITHOUT the lo*lo' term i*j/2^24 that the
                       true product has. All sums are multiples of 2^-12 below 2^12: exact in fp32.
               i is not widened below -7: under 1.0 bf16's spacing halves to 2^-8 and 1 - 8/4096 is a tie.
  float_case   N(0, 1) entries everywhere (scaled entries such as 2^U(-4,4) let one product dominate and put
               the emulation itself at the project's bound; they are not used).

Epilogues (`epilogue`): kind in bias / gelu / dgelu / relu / relu_train / rowadd / addln, stated once over a
dtype: float64 is the reference, float32 the "fp32 restatement" of tests/test_gpu_glue.py's comparison rule,
with the operations in the kernels' order (v * scale then + x; aux from the undropped value), so that on
exact pre-activations the fp32 restatement is what a correct kernel returns bit for bit - except GELU, whose
erf / exp differ between implementations (`gelu_exact_bound`).
"""
from __future__ import annotations

import functools
import math

import numpy as np
import torch

from tests import dropout_ref as D

F32, F64 = torch.float32, torch.float64

# public epilogue numbers of rsx_gemm_x3_form: 0..3 as rsx_gemm_x3, 4 = rsx_gemm_x3_relu_train
EPI = {"bias": 0, "gelu": 1, "dgelu": 2, "relu": 3, "relu_train": 4}
FORM_WS, FORM_TWO, FORM_FOUR32, FORM_FOUR16, FORM_SPLIT = 0, 1, 2, 3, 4
SEED = (0x9E3779B9 << 32) | 0x7F4A7C15   # both seed words take part in the mask


# ------------------------------------------------------------------------------------ operands
def int_case(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    a = torch.randint(-3, 4, (M, K), generator=g).float()
    w = torch.randint(-2, 3, (N, K), generator=g).float()
    b = torch.randint(-4, 4, (N,), generator=g).float() + 0.5    # half-integers: z is never 0
    return a, w, b


def _lo_side(rows, K, g):
    return 1.0 + torch.randint(-7, 8, (rows, K), generator=g).float() / 4096.0


def _sign_side(rows, K, g):
    return torch.randint(-1, 2, (rows, K), generator=g).float()


def probe_case(which, M, N, K, seed):
    """(a, w, bias, z64): z64 = the documented three-term sum + bias in float64 (fp32-representable)."""
    g = torch.Generator().manual_seed(seed)
    a = _lo_side(M, K, g) if which in ("a", "ab") else _sign_side(M, K, g)
    w = _lo_side(N, K, g) if which in ("b", "ab") else _sign_side(N, K, g)
    b = torch.randint(-4, 4, (N,), generator=g).float() + 0.5
    z = three_term64(a, w) + b.double()
    return a, w, b, z


def float_case(M, N, K, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(M, K, generator=g), torch.randn(N, K, generator=g), torch.randn(N, generator=g)


# ------------------------------------------------------------------------------------ the bf16x3 product
def split(x):
    """rsx_x3.h: hi = bf16(x), lo = bf16(x - hi), both returned as fp32."""
    hi = x.to(torch.bfloat16).float()
    lo = (x - hi).to(torch.bfloat16).float()
    return hi, lo


def three_term64(a, w):
    """hi*hi' + hi*lo' + lo*hi' summed in float64."""
    ah, al = (t.double() for t in split(a))
    wh, wl = (t.double() for t in split(w))
    out = ah @ wh.T
    if wl.any():
        out += ah @ wl.T
    if al.any():
        out += al @ wh.T
    return out


def emulate32(a, w):
    """The bf16x3 product in fp32: the split, then three fp32 matmuls (the kernel's terms, smallest first)."""
    ah, al = split(a)
    wh, wl = split(w)
    return (al @ wh.T + ah @ wl.T) + ah @ wh.T


def hi_only64(a, w):
    return split(a)[0].double() @ split(w)[0].double().T


def absprod(a, w):
    return a.double().abs() @ w.double().abs().T


def bound(a, w):
    """The project's per-element bound on a bf16x3 GEMM output (tests/test_gpu_kernels.py)."""
    return 2e-5 * absprod(a, w) + 1e-6


# ------------------------------------------------------------------------------------ epilogues
@functools.lru_cache(maxsize=4)
def keep_mask(seed, p, M, N):
    """The host keep mask over m * N + n (shared, read-only)."""
    return torch.from_numpy(D.keep(seed, p, D.gemm_index(M, N)))


def scale_of(p, dt):
    """make_dropout's keep scale: fp32 as the kernel holds it, or its real value 1 / (1 - fp32(p))."""
    if dt == F32:
        return torch.tensor(D.scale32(p))
    p32 = float(np.float32(p))
    return torch.tensor(1.0 / (1.0 - p32) if p32 > 0 else 1.0, dtype=F64)


def gelu_cdf(z):
    return 0.5 * (1.0 + torch.erf(z / math.sqrt(2.0)))


def gelu(z):
    return z * gelu_cdf(z)


def gelu_grad(z):
    return gelu_cdf(z) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def layer_norm(s, ln_w, ln_b, eps):
    """(y, mean, rstd) of rows of s in s.dtype: biased variance, eps inside the root."""
    dt = s.dtype
    mean = s.mean(-1)
    d = s - mean[:, None]
    var = (d * d).mean(-1)
    rstd = 1.0 / torch.sqrt(var + torch.tensor(eps, dtype=dt))
    return d * rstd[:, None] * ln_w.to(dt) + ln_b.to(dt), mean, rstd


def epilogue(kind, acc, dt, bias=None, p=0.0, seed=SEED, aux=None, table=None, ridx=None, x=None):
    """(C, aux_out) of the epilogue `kind` over the raw product acc [M, N], computed in dtype dt.
    aux: dgelu's saved multiplier; table / ridx: rowadd; x: addln's residual (C = s; LayerNorm is separate)."""
    M, N = acc.shape
    v = acc.to(dt)
    if bias is not None and kind != "dgelu":
        v = v + bias.to(dt)
    aux_out = None
    if kind == "gelu":
        aux_out = gelu_grad(v)
        v = gelu(v)
    elif kind == "dgelu":
        v = v * aux.to(dt)
    elif kind == "relu":
        v = torch.clamp_min(v, 0.0)
    elif kind == "relu_train":
        aux_out = (v > 0).to(dt)
        v = torch.clamp_min(v, 0.0)
    elif kind == "rowadd":
        v = v + table.to(dt)[ridx]
    if kind in ("gelu", "dgelu", "relu_train", "addln") and p > 0:
        v = torch.where(keep_mask(seed, p, M, N), v * scale_of(p, dt), torch.zeros((), dtype=dt))
    if kind == "addln":
        v = v + x.to(dt)
    return v, aux_out


def gelu_exact_bound(ref64, p=0.0):
    """|kernel - float64| allowed for gelu / gelu' / their kept, scaled values on an EXACT pre-activation:
    the project's 2e-6 for the function itself (csrc/gemm_x3.hip: 4.2e-7 measured for the branch-free pair,
    torch's own fp32 gelu 1.2e-6), scaled with the kept value, plus three fp32 roundings of the result
    (z * cdf, the fp32 keep scale, the product with it)."""
    return 2e-6 * scale_of(p, F64).item() + 3 * 2.0 ** -24 * ref64.abs()


# ------------------------------------------------------------------------------------ forms
def split_count(M, N, K, cus=256):
    """split_plan's S: fewer 128 x 128 tiles than CUs, S in (8, 4, 3, 2) with K % (32 S) == 0, K / S >= 256
    and tiles * S <= 4 CUs; 1 = no split."""
    tiles = (M + 127) // 128 * (N // 128)
    if K in (128, 256, 384) or tiles >= cus:
        return 1
    for S in (8, 4, 3, 2):
        if K % (S * 32) == 0 and K // S >= 256 and tiles * S <= 4 * cus:
            return S
    return 1


STREAM_EPIS = ("bias", "gelu", "dgelu", "relu", "relu_train")
WS_NT_EPIS = STREAM_EPIS + ("gelu_noaux",)


def form_table():
    """[(group, M, N, K, epi name, with_ws, form, S)] at 256 CUs: every row of the issue's table that goes
    through rsx_gemm_x3_form (the tn / rowadd / addln entries are weight-stationary by construction)."""
    rows = []
    for K in (16, 32, 48, 96):
        for e in STREAM_EPIS:
            for N in (128, 256):
                for M in (1, 127, 128, 129, 257):
                    rows.append(("two", M, N, K, e, True, FORM_TWO, 0))
    rows.append(("two_big", 2049, 2048, 512, "bias", True, FORM_TWO, 0))
    for K, ws in ((288, True), (320, True), (352, True), (544, True), (512, False)):
        for e in STREAM_EPIS:
            for N in (128, 256):
                for M in (1, 129, 257):
                    rows.append(("four32", M, N, K, e, ws, FORM_TWO if e == "dgelu" else FORM_FOUR32, 0))
    for K in (272, 304):
        for e in ("bias", "gelu"):
            for M in (1, 129):
                rows.append(("four16", M, 128, K, e, True, FORM_FOUR16, 0))
    for K, S in ((512, 2), (768, 3), (1024, 4), (2048, 8)):
        for e in STREAM_EPIS:
            for N in (128, 256):
                for M in (1, 129):
                    rows.append(("split", M, N, K, e, True, FORM_SPLIT, S))
    for K in (128, 256, 384):
        for e in STREAM_EPIS:
            for N in (128, 384):
                for M in (1, 31, 32, 33, 127, 129):
                    rows.append(("ws", M, N, K, e, True, FORM_WS, 0))
    return rows


def strip_rows(cus, N, K):
    """The smallest M at which some waves of gemm_ws_k own three 32-row strips and the rest two:
    2 * 128 * (CUs / nblk) + 33 (a workgroup's four waves take 128 rows per round; nblk column blocks of
    128 columns, 64 at K = 384)."""
    nblk = N // (64 if K == 384 else 128)
    return 2 * 128 * max(cus // nblk, 1) + 33
