"""Host-side argument checks of the raw-pointer wrappers in recsys_amd.ops.

Every call here must be refused on the host before any kernel launch: TypeError for a wrong
dtype, ValueError for a wrong shape or length, RuntimeError for a tensor on another device.
Only CPU (and storage-less "meta") tensors are used, so nothing can reach a kernel; a call whose
arguments are all consistent still ends in ensure_device's RuntimeError (no CPU path).
"""
import types

import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import ops

D = 64


def f(*shape):
    return torch.zeros(*shape)


def meta(*shape, dtype=torch.float32):
    return torch.empty(*shape, dtype=dtype, device="meta")


def li(n, dtype=torch.int64):
    return torch.zeros(n, dtype=dtype)


def _embeddings(word=None):
    ns = types.SimpleNamespace
    return ns(word_embeddings=ns(weight=f(10, 256) if word is None else word),
              position_embeddings=ns(weight=f(8, 256)), token_type_embeddings=ns(weight=f(2, 256)),
              LayerNorm=ns(weight=f(256), bias=f(256), eps=1e-12), dropout=ns(p=0.0), training=False)


# every (x, res, weight, bias) LayerNorm-family wrapper behind one call shape
LN = {
    "layer_norm": lambda x, r, w, b: ops.layer_norm(x, w, b),
    "layer_norm_pass": lambda x, r, w, b: ops.layer_norm_pass(x, w, b),
    "add_layer_norm": lambda x, r, w, b: ops.add_layer_norm(x, r, w, b),
    "add_layer_norm_infer": lambda x, r, w, b: ops.add_layer_norm_infer(x, r, w, b),
    "add_dropout": lambda x, r, w, b: ops.add_dropout(x, r, 0.1),
}
HAS_RES = ("add_layer_norm", "add_layer_norm_infer", "add_dropout")
HAS_W = ("layer_norm", "layer_norm_pass", "add_layer_norm", "add_layer_norm_infer")


@pytest.mark.parametrize("name", sorted(LN))
def test_ln_family_x_dtype(name):
    with pytest.raises(TypeError, match="float32"):
        LN[name](f(3, D).double(), f(3, D).double(), f(D), f(D))


@pytest.mark.parametrize("name", HAS_RES)
def test_ln_family_res_dtype_shape_device(name):
    with pytest.raises(TypeError, match="res"):
        LN[name](f(3, D), f(3, D).half(), f(D), f(D))
    with pytest.raises(ValueError, match="res"):
        LN[name](f(3, D), f(4, D), f(D), f(D))
    with pytest.raises(RuntimeError, match="res"):
        LN[name](f(3, D), meta(3, D), f(D), f(D))


@pytest.mark.parametrize("name", HAS_W)
def test_ln_family_weight_bias(name):
    with pytest.raises(ValueError, match="weight"):
        LN[name](f(3, D), f(3, D), f(D + 4), f(D))
    with pytest.raises(ValueError, match="bias"):
        LN[name](f(3, D), f(3, D), f(D), f(D - 4))
    with pytest.raises(TypeError, match="weight"):
        LN[name](f(3, D), f(3, D), f(D).double(), f(D))
    with pytest.raises(TypeError, match="bias"):
        LN[name](f(3, D), f(3, D), f(D), f(D).to(torch.bfloat16))
    with pytest.raises(RuntimeError, match="weight"):
        LN[name](f(3, D), f(3, D), meta(D), f(D))
    with pytest.raises(RuntimeError, match="bias"):
        LN[name](f(3, D), f(3, D), f(D), meta(D))


@pytest.mark.parametrize("name", sorted(LN))
def test_ln_family_consistent_cpu_call_still_refused(name):
    """The checks pass, then ensure_device refuses the CPU tensor: no CPU path."""
    with pytest.raises(RuntimeError, match="ROCm GPU tensor"):
        LN[name](f(3, D), f(3, D), f(D), f(D))


def test_gather_rows_index():
    src = f(10, D)
    with pytest.raises(TypeError, match="idx"):
        ops.gather_rows(src, torch.zeros(4))
    with pytest.raises(TypeError, match="idx"):
        ops.gather_rows(src, torch.zeros(4, dtype=torch.bool))
    with pytest.raises(RuntimeError, match="idx"):
        ops.gather_rows(src, meta(4, dtype=torch.int64))
    with pytest.raises(TypeError, match="floating-point"):
        ops.gather_rows(li(10), li(4))


def test_gather_rows_int32_index_is_converted(monkeypatch):
    """An int32 idx reaches the autograd function as int64 (the kernel reads 8-byte indices)."""
    seen = {}

    def fake_apply(src, idx, *rest):
        seen["dtype"] = idx.dtype
        raise RuntimeError("stop before the launch")

    monkeypatch.setattr(ops._GatherRows, "apply", staticmethod(fake_apply))
    with pytest.raises(RuntimeError, match="stop before"):
        ops.gather_rows(f(10, D), torch.tensor([1, 2, 3], dtype=torch.int32))
    assert seen["dtype"] == torch.int64


def test_gather_rows_multi():
    src = f(10, D)
    ok = li(3)
    with pytest.raises(TypeError, match=r"idx\[1\]"):
        ops.gather_rows_multi(src, [(ok, True), (torch.zeros(3), False)])
    with pytest.raises(RuntimeError, match=r"idx\[0\]"):
        ops.gather_rows_multi(src, [(meta(3, dtype=torch.int64), True)])
    with pytest.raises(TypeError, match="src"):
        ops.gather_rows_multi(src.double(), [(ok, True)])
    with pytest.raises(ValueError, match="src"):
        ops.gather_rows_multi(f(2, 5, D), [(ok, True)])
    seen = {}

    class Stop(Exception):
        pass

    def fake_apply(src, norms, eps, *idxs):
        seen["dtypes"] = [i.dtype for i in idxs]
        raise Stop

    orig = ops._GatherRowsMulti.apply
    ops._GatherRowsMulti.apply = staticmethod(fake_apply)
    try:
        with pytest.raises(Stop):
            ops.gather_rows_multi(src, [(li(3, torch.int32), True), (li(2, torch.uint8), False)])
    finally:
        ops._GatherRowsMulti.apply = orig
    assert seen["dtypes"] == [torch.int64, torch.int64]


def test_segment_mean():
    x, seg, tok, cnt = f(7, D), li(4), li(7), f(3)
    with pytest.raises(TypeError, match="x"):
        ops.segment_mean(x.double(), seg, tok, cnt)
    with pytest.raises(ValueError, match="x"):
        ops.segment_mean(f(7), seg, tok, cnt)
    with pytest.raises(TypeError, match="seg"):
        ops.segment_mean(x, seg.float(), tok, cnt)
    with pytest.raises(TypeError, match="tok_seg"):
        ops.segment_mean(x, seg, tok.double(), cnt)
    with pytest.raises(ValueError, match="seg"):
        ops.segment_mean(x, li(3), tok, cnt)           # offsets must number counts + 1
    with pytest.raises(ValueError, match="tok_seg"):
        ops.segment_mean(x, seg, li(6), cnt)           # one segment id per row of x
    with pytest.raises(RuntimeError, match="seg"):
        ops.segment_mean(x, meta(4, dtype=torch.int64), tok, cnt)
    with pytest.raises(RuntimeError, match="tok_seg"):
        ops.segment_mean(x, seg, meta(7, dtype=torch.int64), cnt)
    with pytest.raises(RuntimeError, match="counts"):
        ops.segment_mean(x, seg, tok, meta(3))
    with pytest.raises(RuntimeError, match="ROCm GPU tensor"):
        ops.segment_mean(x, seg.int(), tok.int(), cnt)  # int32 offsets are converted, then no CPU path


def test_crossnet():
    x = f(5, 8)
    ks, bs = [f(8, 1), f(8, 1)], [f(8), f(8)]
    with pytest.raises(TypeError, match="x"):
        ops.crossnet(x.double(), ks, bs, want_x=True)
    with pytest.raises(ValueError, match="x"):
        ops.crossnet(f(8), ks, bs, want_x=True)
    with pytest.raises(ValueError, match="biases"):
        ops.crossnet(x, ks, bs[:1], want_x=True)
    with pytest.raises(ValueError, match=r"kernels\[1\]"):
        ops.crossnet(x, [f(8, 1), f(4, 1)], bs, want_x=True)
    with pytest.raises(ValueError, match=r"biases\[0\]"):
        ops.crossnet(x, ks, [f(12), f(8)], want_x=True)
    with pytest.raises(TypeError, match=r"kernels\[0\]"):
        ops.crossnet(x, [f(8, 1).double(), f(8, 1)], bs, want_x=True)
    with pytest.raises(TypeError, match=r"biases\[1\]"):
        ops.crossnet(x, ks, [f(8), f(8).half()], want_x=True)
    with pytest.raises(RuntimeError, match=r"kernels\[0\]"):
        ops.crossnet(x, [meta(8, 1), f(8, 1)], bs, want_x=True)
    with pytest.raises(RuntimeError, match=r"biases\[1\]"):
        ops.crossnet(x, ks, [f(8), meta(8)], want_x=True)
    with pytest.raises(ValueError, match="w_head"):
        ops.crossnet(x, ks, bs, w_head=f(16))
    with pytest.raises(TypeError, match="w_head"):
        ops.crossnet(x, ks, bs, w_head=f(8).double())
    with pytest.raises(RuntimeError, match="w_head"):
        ops.crossnet(x, ks, bs, w_head=meta(8))
    with pytest.raises(RuntimeError, match="ROCm GPU tensor"):
        ops.crossnet(x, ks, bs, w_head=f(8))


def test_linear():
    x, w, b = f(5, 16), f(8, 16), f(8)
    with pytest.raises(TypeError, match="x"):
        ops.linear(x.double(), w, b)
    with pytest.raises(ValueError, match="x"):
        ops.linear(f(2, 5, 16), w, b)
    with pytest.raises(TypeError, match="weight"):
        ops.linear(x, w.half(), b)
    with pytest.raises(ValueError, match="weight"):
        ops.linear(x, f(8, 12), b)
    with pytest.raises(ValueError, match="weight"):
        ops.linear(x, f(16), b)
    with pytest.raises(RuntimeError, match="weight"):
        ops.linear(x, meta(8, 16), b)
    with pytest.raises(TypeError, match="bias"):
        ops.linear(x, w, b.double())
    with pytest.raises(ValueError, match="bias"):
        ops.linear(x, w, f(16))
    with pytest.raises(RuntimeError, match="bias"):
        ops.linear(x, w, meta(8))
    with pytest.raises(RuntimeError, match="ROCm GPU tensor"):
        ops.linear(x, w, b)


def test_loss_combine():
    s = torch.zeros(())
    with pytest.raises(ValueError, match="s_un"):
        ops.loss_combine(s, None, s, s, 4, 2, 0.1, 0.2)
    with pytest.raises(TypeError, match="s_un"):
        ops.loss_combine(s, s.double(), s, s, 4, 2, 0.1, 0.2)
    with pytest.raises(TypeError, match="s_main"):
        ops.loss_combine(s.double(), s, s, s, 4, 2, 0.1, 0.2)
    with pytest.raises(TypeError, match="s_sup"):
        ops.loss_combine(s, s, s.half(), s, 4, 2, 0.1, 0.2)
    with pytest.raises(TypeError, match="cnt"):
        ops.loss_combine(s, s, s, torch.zeros((), dtype=torch.int64), 4, 2, 0.1, 0.2)
    with pytest.raises(ValueError, match="s_un"):
        ops.loss_combine(s, f(2), s, s, 4, 2, 0.1, 0.2)
    with pytest.raises(ValueError, match="s_main"):
        ops.loss_combine(f(3), s, s, s, 4, 2, 0.1, 0.2)
    with pytest.raises(ValueError, match="s_sup"):
        ops.loss_combine(s, s, f(0), s, 4, 2, 0.1, 0.2)
    with pytest.raises(ValueError, match="cnt"):
        ops.loss_combine(s, s, s, f(2), 4, 2, 0.1, 0.2)
    with pytest.raises(RuntimeError, match="s_main"):
        ops.loss_combine(meta(1), s, s, s, 4, 2, 0.1, 0.2)
    with pytest.raises(RuntimeError, match="s_sup"):
        ops.loss_combine(s, s, meta(1), s, 4, 2, 0.1, 0.2)
    with pytest.raises(RuntimeError, match="cnt"):
        ops.loss_combine(s, s, s, meta(1), 4, 2, 0.1, 0.2)
    with pytest.raises(RuntimeError, match="ROCm GPU tensor"):
        ops.loss_combine(None, s, None, None, 0, 2, 0.1, 0.2)


def test_bert_embed_packed():
    emb = _embeddings()
    with pytest.raises(TypeError, match="ids"):
        ops.bert_embed_packed(emb, torch.zeros(5), li(5))
    with pytest.raises(TypeError, match="tok_pos"):
        ops.bert_embed_packed(emb, li(5), torch.zeros(5))
    with pytest.raises(ValueError, match="tok_pos"):
        ops.bert_embed_packed(emb, li(5), li(4))
    with pytest.raises(RuntimeError, match="ids"):
        ops.bert_embed_packed(emb, meta(5, dtype=torch.int64), li(5))
    with pytest.raises(RuntimeError, match="tok_pos"):
        ops.bert_embed_packed(emb, li(5), meta(5, dtype=torch.int64))
    with pytest.raises(RuntimeError, match="ROCm GPU tensor"):
        ops.bert_embed_packed(emb, li(5, torch.int32), li(5, torch.int16))   # converted, then no CPU path
