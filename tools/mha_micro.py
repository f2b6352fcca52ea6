"""Micro-benchmark of the causal attention kernels at the bench shape (4096 users, H&M-shaped
lengths, H=4, Dh=32): packed with dropout 0.2 (the training step), packed without dropout,
and dense [T/50, 50] (no segment search). Prints avg ms of forward and forward+backward. `legs` holds
the other shapes, one per remaining kernel of mha.hip: the item tower's 16 unmasked tokens, BERT's head
dim 64 packed, the fp32 kernels and the fused in_proj + attention forward.

  python tools/mha_micro.py
"""
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_amd  # noqa: E402,F401
from recsys_amd import ops, synth  # noqa: E402
from recsys_amd.tower_code.v1_refine_usertower import PackedTokens  # noqa: E402


def bench(fn, n=10):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return round(e0.elapsed_time(e1) / n, 4)


def main():
    dev = torch.device("cuda", 0)
    items = synth.make_items(seed=0)
    b = synth.make_batch(items, int(os.environ.get("BATCH", "8192")), seed=100)
    pk = PackedTokens(b["padding_mask"].to(dev))
    T = pk.flat.numel()
    g = torch.Generator(device="cpu").manual_seed(0)
    qkv = torch.randn(T, 384, generator=g).to(dev).requires_grad_()
    gy = torch.randn(T, 128, generator=g).to(dev)
    res = {"tokens": T}
    for p in (0.2, 0.0):
        f = lambda: ops.mha(qkv, pk.tok_pad, 4, causal=True, p_drop=p, seg_off=pk.seg_off)
        res[f"packed_p{p}_fwd_ms"] = bench(f)
        res[f"packed_p{p}_fwdbwd_ms"] = bench(lambda: torch.autograd.grad(f(), qkv, gy))
    Bd = T // 50
    qd = qkv.detach()[:Bd * 50].reshape(Bd, 50, 384).clone().requires_grad_()
    gd = gy[:Bd * 50].reshape(Bd, 50, 128)
    fd = lambda: ops.mha(qd, None, 4, causal=True, p_drop=0.2)
    res["dense_fwd_ms"] = bench(fd)
    res["dense_fwdbwd_ms"] = bench(lambda: torch.autograd.grad(fd(), qd, gd))
    res["legs"] = other_legs(dev, qkv, gy, pk)
    print(json.dumps(res), flush=True)


def other_legs(dev, qkv, gy, pk):
    """The shapes that reach the other kernels of mha.hip, each at the batch of the bench.py leg that runs
    its model (named in `leg`); `kernels` = forward, backward."""
    import numpy as np
    g = torch.Generator(device="cpu").manual_seed(1)
    legs = {}

    def case(name, leg, kernels, D, H, B, lens, causal, p, prec="bf16x3", fwd_only=False):
        prev = ops.mha_precision()
        ops.set_mha_precision(prec)
        try:
            if isinstance(lens, int):  # dense [B, lens] tokens
                q = torch.randn(B, lens, 3 * D, generator=g).to(dev).requires_grad_()
                gr = torch.randn(B, lens, D, generator=g).to(dev)
                f = lambda: ops.mha(q, None, H, causal=causal, p_drop=p)
                tokens = B * lens
            else:  # packed segments
                off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)
                tokens = int(off[-1])
                q = torch.randn(tokens, 3 * D, generator=g).to(dev).requires_grad_()
                gr = torch.randn(tokens, D, generator=g).to(dev)
                f = lambda: ops.mha(q, None, H, causal=causal, p_drop=p, seg_off=off, max_len=int(max(lens)))
            r = {"leg": leg, "kernels": kernels, "tokens": tokens, "fwd_ms": bench(f, 400)}
            if not fwd_only:
                r["fwdbwd_ms"] = bench(lambda: torch.autograd.grad(f(), q, gr), 400)
            legs[name] = r
        finally:
            ops.set_mha_precision(prev)

    rng = np.random.default_rng(21)
    simcse = "bench_simcse_train (B = 192 items per view)"
    case("item_tower_16tok", simcse, "mha_fwd_x3b_k, mha_bwd_x3p_k", 128, 4, 192, 16, False, 0.1)
    case("bert_dh64_len32", simcse + ", text lengths U{2..32}", "mha_fwd_x3b64_k, mha_bwd64_k<32>", 768, 12, 192,
         rng.integers(2, 33, 192), False, 0.1)
    case("bert_dh64_refresh", "bench_item_refresh (768 products, text lengths U{2..32}), forward only",
         "mha_fwd_x3b64_k", 768, 12, 768, rng.integers(2, 33, 768), False, 0.0, fwd_only=True)
    case("bert_dh64_len64", "no bench leg runs lengths above 32: the SimCSE batch with lengths U{2..64}",
         "mha_fwd_x3b64_k, mha_bwd64_k<64>", 768, 12, 192, rng.integers(2, 65, 192), False, 0.1)
    case("item_tower_dh16_fp32", "bench_item_tower (256 items, d = 64), backward added",
         "mha_fwd_k<16>, mha_bwd_k<16>", 64, 4, 256, 16, False, 0.1, prec="fp32")
    # the headline's packed tokens in fp32 (the tests' second opinion) and through the fused in_proj + attention
    f32 = lambda: ops.mha(qkv, pk.tok_pad, 4, causal=True, p_drop=0.2, seg_off=pk.seg_off)
    ops.set_mha_precision("fp32")
    try:
        legs["headline_fp32"] = {"leg": "the headline step's tokens, RSX_MHA_PRECISION=fp32",
                                 "kernels": "mha_fwd_k<32>, mha_bwd_mfma_k", "fwd_ms": bench(f32),
                                 "fwdbwd_ms": bench(lambda: torch.autograd.grad(f32(), qkv, gy))}
    finally:
        ops.set_mha_precision("bf16x3")
    x = torch.randn(qkv.shape[0], 128, generator=g).to(dev)
    w = (torch.randn(384, 128, generator=g) / 128 ** 0.5).to(dev)
    b = torch.randn(384, generator=g).to(dev)
    with torch.no_grad():
        fq = lambda: ops._QKVMHA.apply(x, w, b, pk.tok_pad, pk.seg_off.to(torch.int32), 4, True, 0.2, 12345)
        legs["headline_fused_fwd"] = {"leg": "the headline step's tokens through rsx_mha_qkv_fwd_x3, forward only",
                                      "kernels": "mha_qkv_fwd_x3_k<4>", "fwd_ms": bench(fq)}
    return legs


if __name__ == "__main__":
    main()
