"""Micro-benchmark of the DCN-V2 RankingModel training step at 65,536 rows x 276 columns (user 128 +
item 128 + context 20): the native step (RankingModel.make_trainer().step) against the same step in
plain PyTorch on the same GPU (the module tree's own autograd forward with dropout 0.2,
binary_cross_entropy_with_logits, torch.optim.AdamW). Event timing, warm-up first, median over
--iters steps on fresh batches, plus the native step's phases (ops.timed). Also rsx_crossnet_bwd
alone (with and without dx) and rsx_crossnet's head-only forward by HIP events over --reps
back-to-back calls, against their byte models and DESIGN.md section 4's 8 TB/s HBM figure:
  backward with dx  B*D*4 read + B*4 read + B*D*4 written; without dx the reads only;
  forward           B*D*4 read + B*4 written.
Writes --out (profiles/dcn_train_micro.json). --only-step: just --iters native steps (for
rocprofv3 --kernel-trace --stats)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_amd  # noqa: E402,F401
from recsys_amd import ops  # noqa: E402
from recsys_amd.temp_model.ranker_skelet import RankingModel  # noqa: E402

HBM_BYTES_PER_S = 8e12


class TorchRankingModel(nn.Module):
    """The same module tree trained by autograd: cross layers as x0 * (xl @ k + b) + xl, the deep
    Sequential (dropout active in train mode), final_head on cat(cross, deep); returns logits."""

    def __init__(self, src: RankingModel):
        super().__init__()
        self.kernels = nn.ParameterList([nn.Parameter(k.detach().clone()) for k in src.cross_net.kernels])
        self.biases = nn.ParameterList([nn.Parameter(b.detach().clone()) for b in src.cross_net.biases])
        d = src.deep_net
        self.deep = nn.Sequential(nn.Linear(d[0].in_features, 256), nn.LayerNorm(256), nn.GELU(), nn.Dropout(d[3].p),
                                  nn.Linear(256, 128), nn.LayerNorm(128), nn.GELU())
        self.head = nn.Linear(d[0].in_features + 128, 1)

    def forward(self, user, item, ctx):
        x = torch.cat([user, item, ctx], 1)
        xl = x
        for k, b in zip(self.kernels, self.biases):
            xl = x * (xl @ k + b) + xl
        return self.head(torch.cat([xl, self.deep(x)], 1)).squeeze(1)


def batches(rows, count, dev, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(count):
        parts = [F.normalize(torch.randn(rows, 128, generator=g), dim=1) for _ in range(2)]
        parts.append(torch.randn(rows, 20, generator=g) * 0.1)
        y = (torch.rand(rows, generator=g) < 0.4).float()
        out.append(tuple(t.to(dev) for t in parts + [y]))
    return out


def time_steps(step, data, warmup, iters):
    for i in range(warmup):
        step(*data[i % len(data)])
    torch.cuda.synchronize()
    ms = []
    for i in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step(*data[(warmup + i) % len(data)])
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def time_kernel(fn, reps, rounds=5):
    """Median over rounds of (time of reps back-to-back calls) / reps, in ms."""
    fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            fn()
        e1.record()
        e1.synchronize()
        out.append(e0.elapsed_time(e1) / reps)
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--only-step", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "dcn_train_micro.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    model = RankingModel().to(dev)
    D = model.deep_net[0].in_features
    data = batches(a.rows, 4, dev, seed=3)
    tr = model.make_trainer(lr=1e-3)

    def native_step(user, item, ctx, y):
        return tr.step(user, item, ctx, y)

    if a.only_step:
        for i in range(a.warmup + a.iters):
            native_step(*data[i % len(data)])
        torch.cuda.synchronize()
        return
    result = {"rows": a.rows, "columns": D, "iters": a.iters, "warmup": a.warmup, "reps": a.reps,
              "device": torch.cuda.get_device_name(0)}
    ref = TorchRankingModel(model).to(dev).train()
    med, best = time_steps(native_step, data, a.warmup, a.iters)
    ops.timing_start()
    for i in range(a.iters):
        native_step(*data[i % len(data)])
    phases = {k: v[1] / a.iters for k, v in ops.timing_stop().items()
              if k.startswith("dcn_train/") or k == "crossnet_bwd"}
    result["native"] = {"median_ms": med, "min_ms": best, "phase_ms": phases}
    print(f"native: median {med:.3f} ms, phases {phases}", flush=True)

    opt = torch.optim.AdamW(ref.parameters(), lr=1e-3)

    def torch_step(user, item, ctx, y):
        opt.zero_grad(set_to_none=True)
        loss = F.binary_cross_entropy_with_logits(ref(user, item, ctx), y)
        loss.backward()
        opt.step()
        return loss

    med_t, best_t = time_steps(torch_step, data, a.warmup, a.iters)
    result["torch"] = {"median_ms": med_t, "min_ms": best_t}
    result["speedup"] = med_t / med
    print(f"torch: median {med_t:.3f} ms; native is {med_t / med:.2f}x", flush=True)

    # the cross-network kernels alone
    B = a.rows
    x = torch.cat(data[0][:3], 1).contiguous()
    ks, bs = list(model.cross_net.kernels), list(model.cross_net.biases)
    wh = model.final_head.weight.detach().reshape(-1)[:D].contiguous()
    g = torch.randn(B, device=dev) / B
    # raw C-ABI calls on preallocated buffers: the wrappers' host time (allocations, pointer arrays)
    # would exceed the kernels' own at this size
    from recsys_amd import _native as N
    lib, L = N.lib(), len(ks)
    kf, bf = [k.detach().reshape(-1).contiguous() for k in ks], [b.detach().contiguous() for b in bs]
    kp, bp = N.ptr_array(kf), N.ptr_array(bf)
    grads = torch.empty(2 * L + 1, D, device=dev)
    dkp, dbp = N.ptr_array([grads[l] for l in range(L)]), N.ptr_array([grads[L + l] for l in range(L)])
    dx, part = torch.empty(B, D, device=dev), torch.empty(B, device=dev)
    nws = lib.rsx_crossnet_bwd_workspace_bytes(B, D, L, 0)
    ws = torch.empty(nws, device=dev, dtype=torch.uint8)
    st = N.stream()

    def bwd(with_dx):
        N.check(lib.rsx_crossnet_bwd(N.ptr(x), D, B, D, L, kp, bp, N.ptr(wh), N.ptr(g), None, dkp, dbp,
                                     N.ptr(grads[2 * L]), N.ptr(dx) if with_dx else None, N.ptr(ws), nws, 0, st),
                "crossnet_bwd")

    def fwd():
        N.check(lib.rsx_crossnet(N.ptr(x), D, B, D, L, kp, bp, N.ptr(wh), None, N.ptr(part), st), "crossnet")

    t_dx = time_kernel(lambda: bwd(True), a.reps)
    t_nodx = time_kernel(lambda: bwd(False), a.reps)
    t_fwd = time_kernel(fwd, a.reps)
    rows = {"bwd_with_dx": (t_dx, B * D * 4 + B * 4 + B * D * 4), "bwd_without_dx": (t_nodx, B * D * 4 + B * 4),
            "fwd_head_only": (t_fwd, B * D * 4 + B * 4)}
    result["crossnet"] = {k: {"ms": t, "model_bytes": nb, "gbytes_per_s": nb / (t * 1e-3) / 1e9,
                              "fraction_of_hbm": nb / (t * 1e-3) / HBM_BYTES_PER_S} for k, (t, nb) in rows.items()}
    print(json.dumps(result["crossnet"]), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
