"""Inputs, float64 reference and deliberately wrong variants of the DeepFM rerank forward (CPU, torch only;
test infrastructure for tests/test_deepfm_fwd_ref_cpu.py and tests/test_gpu_deepfm_forms.py).

Input scale: V and first-order entries ~ N(0, 0.1^2), w1 = randn / sqrt(16 F) / 0.1 (h1 ~ N(0, 1)),
w2 = randn / 16, wo = randn / 11, biases ~ N(0, 0.5^2). At this scale the logits have std 0.4-2, a
correct bf16x3 kernel is ~1e-5 from float64 and a kernel that drops one `lo` image of a bf16x3 product is
> 1e-3 off: the project's logit bound TOL = 1e-4 separates the two (test_deepfm_fwd_ref_cpu.py asserts it).
"""
import math

import torch

from oracle.deepfm import deepfm_forward

TOL = 1e-4          # |logit - float64 reference|, every row, rtol 0
E, H1, H2 = 16, 256, 128
BIG_VOCAB = 5003    # field 0: much larger than every other field
_BLOCK = 4096       # reference rows per step


def vocab_of(f):
    """Vocabulary of field f: field 0 large, fields 1, 8, 15, ... a single row, the rest 3..99 (all unequal
    to their neighbours, so the last row of a field's table is the last row of nothing else)."""
    if f == 0:
        return BIG_VOCAB
    if f % 7 == 1:
        return 1
    return 3 + (37 * f) % 97


def make_case(F, R, seed):
    """One DeepFM problem on the CPU: per-field tables V[f] [vocab_f, 16] / W[f] [vocab_f], ids x [R, F]
    (row 0 all zeros, row 1 and the last row every field's last id), the (256, 128) DNN and the output bias."""
    g = torch.Generator().manual_seed(seed * 1000 + F)
    vocab = [vocab_of(f) for f in range(F)]
    V = [0.1 * torch.randn(v, E, generator=g) for v in vocab]
    W = [0.1 * torch.randn(v, generator=g) for v in vocab]
    w1 = torch.randn(H1, F * E, generator=g) / math.sqrt(E * F) / 0.1
    b1 = 0.5 * torch.randn(H1, generator=g)
    w2 = torch.randn(H2, H1, generator=g) / 16
    b2 = 0.5 * torch.randn(H2, generator=g)
    wo = torch.randn(H2, generator=g) / 11
    bias = float(0.5 * torch.randn((), generator=g))
    vt = torch.tensor(vocab, dtype=torch.int64)
    x = (torch.rand(R, F, generator=g, dtype=torch.float64) * vt).long().clamp_(max=vt - 1)
    x[0] = 0
    if R > 1:
        x[1] = vt - 1
        x[R - 1] = vt - 1
    return dict(F=F, R=R, seed=seed, vocab=vocab, last=vt - 1, V=V, W=W, x=x, w1=w1, b1=b1, w2=w2, b2=b2, wo=wo,
                bias=bias)


def _x_rows(case, rows):
    x = case["x"]
    return x if rows is None else x[rows]


def reference(case, rows=None, w_null=()):
    """float64 (logit, prob) of the case's rows (all, a slice or an index tensor) through the oracle, in
    row blocks. w_null: fields whose first-order table is absent (a NULL W[f]: it contributes 0)."""
    x = _x_rows(case, rows)
    lin = [torch.zeros_like(w) if f in w_null else w for f, w in enumerate(case["W"])]
    logit = torch.empty(x.shape[0], dtype=torch.float64)
    for lo in range(0, x.shape[0], _BLOCK):
        logit[lo:lo + _BLOCK], _ = deepfm_forward(x[lo:lo + _BLOCK], case["V"], lin, case["bias"],
                                                  [case["w1"], case["w2"]], [case["b1"], case["b2"]], case["wo"])
    return logit, torch.sigmoid(logit)


def reference_fp32(case, rows=None):
    """The oracle in float32 (the reference arithmetic): the floor a correct fp32 kernel sits on."""
    x = _x_rows(case, rows)
    logit, _ = deepfm_forward(x, case["V"], case["W"], case["bias"], [case["w1"], case["w2"]],
                              [case["b1"], case["b2"]], case["wo"], dtype=torch.float32)
    return logit.double()


def lin_reference(case, rows=None, w_null=()):
    """float64 bias + first order + FM (rsx_deepfm_embed's lin_out)."""
    x = _x_rows(case, rows)
    emb, first = _gather(case, x)
    for f in w_null:
        first[:, f] = 0
    return case["bias"] + first.sum(1) + _fm(emb)


# ---- the pieces, restated so that single terms can be dropped -------------------------------------------
def _gather(case, x):
    emb = torch.stack([case["V"][f][x[:, f]] for f in range(case["F"])], dim=1).double()   # [R, F, 16]
    first = torch.stack([case["W"][f][x[:, f]] for f in range(case["F"])], dim=1).double()  # [R, F]
    return emb, first


def _fm(emb):
    return 0.5 * (emb.sum(1) ** 2 - (emb * emb).sum(1)).sum(1)


def _split(t):
    """fp32 value -> (hi, lo) bf16 images as float64, as the kernels build them: hi = bf16(v),
    lo = bf16(v - hi) (the difference is exact in fp32)."""
    t = t.float()
    hi = t.bfloat16().float()
    lo = (t - hi).bfloat16().float()
    return hi.double(), lo.double()


def _x3(a, w, drop=None):
    """a [R, K] x w [N, K]^T as hi.hi + hi.lo + lo.hi in float64; drop = "a" / "w" leaves that lo image out."""
    ah, al = _split(a)
    wh, wl = _split(w)
    out = ah @ wh.T
    if drop != "w":
        out = out + ah @ wl.T
    if drop != "a":
        out = out + al @ wh.T
    return out


def _dnn(case, h, l1=None, l2=None, exact=False):
    """The DNN term in float64. exact: plain products; else bf16x3 products (l1 / l2: the lo image dropped in
    that layer, "a" the activations, "w" the weights), h1 rounded to fp32 before its split as the kernels do."""
    if exact:
        h1 = torch.relu(h @ case["w1"].double().T + case["b1"].double())
        h2 = torch.relu(h1 @ case["w2"].double().T + case["b2"].double())
    else:
        h1 = torch.relu(_x3(h, case["w1"], l1) + case["b1"].double()).float()
        h2 = torch.relu(_x3(h1, case["w2"], l2) + case["b2"].double())
    return h2 @ case["wo"].double()


def bf16x3_model(case, rows=None):
    """float64 emulation of both DNN layers in hi.hi + hi.lo + lo.hi (everything else exact): the error
    floor of a correct kernel. Reporting only."""
    x = _x_rows(case, rows)
    emb, first = _gather(case, x)
    return case["bias"] + first.sum(1) + _fm(emb) + _dnn(case, emb.reshape(x.shape[0], -1))


SHIFT_MUTANT = "row takes the previous row's ids"


def shifted_row(case):
    """The row the row-shift mutant gets wrong (any row whose ids differ from its predecessor's)."""
    return case["R"] // 2


def mutants(case):
    """{name: float64 logits} of the wrong kernels a test has to catch. The lo-dropping ones are the bf16x3
    model with one image left out; the others are exact but for their defect."""
    x = case["x"]
    R, F = x.shape
    emb, first = _gather(case, x)
    h = emb.reshape(R, -1)
    base = case["bias"] + first.sum(1) + _fm(emb)
    out = {
        "x lo dropped in layer 1": base + _dnn(case, h, l1="a"),
        "W1 lo dropped": base + _dnn(case, h, l1="w"),
        "h1 lo dropped in layer 2": base + _dnn(case, h, l2="a"),
        "W2 lo dropped": base + _dnn(case, h, l2="w"),
    }
    dnn = _dnn(case, h, exact=True)
    out["last field missing from the FM term"] = case["bias"] + first.sum(1) + _fm(emb[:, :F - 1]) + dnn
    out["last field missing from the first-order sum"] = case["bias"] + first[:, :F - 1].sum(1) + _fm(emb) + dnn
    out["first-order weight of field 0 missing"] = case["bias"] + first[:, 1:].sum(1) + _fm(emb) + dnn
    r = shifted_row(case)
    if r >= 1:
        xs = x.clone()
        xs[r] = x[r - 1]
        out[SHIFT_MUTANT] = reference(dict(case, x=xs))[0]
    return out
