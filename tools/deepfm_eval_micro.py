"""Micro-benchmark of the binary evaluation: ops.binary_eval alone at R = 65,536 and 1,048,576, and
DeepFM.evaluate at BASELINE configs[2] (39 fields, vocab 1e6/field) over 1,048,576 validation rows,
each against the same computation in plain PyTorch on the same GPU (torch.sort, unique_consecutive
and cumsum for the tie-aware AUC, binary_cross_entropy_with_logits for the Logloss; for evaluate also
the model's forward in torch ops). Every timed call ends with its one host read of the metrics.
Event timing, warm-up first, median over --iters calls on fresh inputs. Also the achieved bytes/s
against DESIGN.md's byte model and the cost of one best-model snapshot copy. Writes --out
(profiles/deepfm_eval_micro.json). --profile-rows R only repeats ops.binary_eval at R, for a kernel trace."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_amd  # noqa: E402,F401
from recsys_amd import ops  # noqa: E402
from recsys_amd.temp_model.ranker_skelet import DeepFM  # noqa: E402

HBM_PEAK = 8e12   # bytes/s


def eval_bytes(R):
    """DESIGN.md's byte model of one rsx_binary_eval: the key pass reads logit and y (8 B a row) and
    writes key + label (5 B); the radix sort reads the keys once for its histograms (4 B) and moves
    the 5-B pairs in and out in each of four 8-bit digit passes (40 B); the two tile passes read the
    sorted pairs (5 B each)."""
    return R * (8 + 5 + 4 + 40 + 5 + 5)


def torch_eval(z, y):
    """(AUC, mean Logloss) in plain PyTorch, tie-aware: the same U2 from the sorted scores' tie groups."""
    zs, idx = torch.sort(z)
    ys = y[idx].to(torch.int64)
    _, cnt = torch.unique_consecutive(zs, return_counts=True)
    last = torch.cumsum(cnt, 0) - 1
    cn = torch.cumsum(1 - ys, 0)[last]       # negatives up to each group's end
    cp = torch.cumsum(ys, 0)[last]
    zero = torch.zeros(1, device=z.device, dtype=torch.int64)
    before = torch.cat([zero, cn[:-1]])
    pos = cp - torch.cat([zero, cp[:-1]])
    u2 = (pos * (before + cn)).sum()
    loss = F.binary_cross_entropy_with_logits(z, y, reduction="sum")
    p, n, u2, loss = torch.stack([cp[-1].double(), cn[-1].double(), u2.double(), loss.double()]).tolist()
    return (u2 / (2 * p * n) if p and n else float("nan")), loss / z.numel(), int(u2)


def torch_logits(model, X, batch):
    """The model's forward in torch ops (embedding lookups, FM, the two-layer DNN), in batches."""
    emb, lin, ws, bs, wo = model._param_lists()
    out = torch.empty(X.shape[0], device=X.device, dtype=torch.float32)
    with torch.no_grad():
        for s in range(0, X.shape[0], batch):
            x = X[s:s + batch]
            v = torch.stack([F.embedding(x[:, f], t) for f, t in enumerate(emb)], dim=1)
            first = sum(F.embedding(x[:, f], t).squeeze(1) for f, t in enumerate(lin))
            fm = 0.5 * (v.sum(1) ** 2 - (v * v).sum(1)).sum(1)
            h = F.relu(F.linear(F.relu(F.linear(v.flatten(1), ws[0], bs[0])), ws[1], bs[1]))
            out[s:s + batch] = model.out.bias + first + fm + F.linear(h, wo).squeeze(1)
    return out


def time_calls(fn, inputs, warmup, iters):
    for i in range(warmup):
        fn(*inputs[i % len(inputs)])
    torch.cuda.synchronize()
    ms = []
    for i in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn(*inputs[(warmup + i) % len(inputs)])
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[65536, 1048576])
    ap.add_argument("--val-rows", type=int, default=1048576)
    ap.add_argument("--fields", type=int, default=39)
    ap.add_argument("--vocab", type=int, default=1_000_000)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "deepfm_eval_micro.json"))
    ap.add_argument("--no-model", action="store_true", help="time ops.binary_eval only")
    ap.add_argument("--profile-rows", type=int, default=0,
                    help="only run ops.binary_eval --iters times at this R (for rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    if a.profile_rows:
        z = torch.from_numpy(rng.standard_normal(a.profile_rows).astype(np.float32)).to(dev)
        y = torch.from_numpy((rng.random(a.profile_rows) < 0.4).astype(np.float32)).to(dev)
        for _ in range(a.warmup + a.iters):
            ops.binary_eval(z, y).result()
        return
    result = {"iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "fields": a.fields,
              "vocab": a.vocab, "val_rows": a.val_rows, "batch": a.batch, "hbm_peak_bytes_per_s": HBM_PEAK}

    for R in a.rows:
        for kind in ("distinct", "one_tie_group"):
            inputs = []
            for _ in range(8):
                z = rng.standard_normal(R).astype(np.float32) if kind == "distinct" else np.full(R, 0.25, np.float32)
                y = (rng.random(R) < 0.4).astype(np.float32)
                inputs.append((torch.from_numpy(z).to(dev), torch.from_numpy(y).to(dev)))
            ref = torch_eval(*inputs[0])
            got = ops.binary_eval(*inputs[0])
            res = got.result()
            assert int(got.counts[2]) == ref[2] and abs(res["logloss"] - ref[1]) < 1e-4, (res, ref)
            nat = time_calls(lambda z, y: ops.binary_eval(z, y).result(), inputs, a.warmup, a.iters)
            enq = time_calls(ops.binary_eval, inputs, a.warmup, a.iters)
            tor = time_calls(torch_eval, inputs, a.warmup, a.iters)
            nbytes = eval_bytes(R)
            result[f"binary_eval_{R}_{kind}"] = {
                "native_ms": nat[0], "native_min_ms": nat[1], "native_without_read_ms": enq[0], "torch_ms": tor[0],
                "torch_min_ms": tor[1], "torch_over_native": tor[0] / nat[0], "model_bytes": nbytes,
                "gbytes_per_s": nbytes / (enq[0] * 1e-3) / 1e9, "fraction_of_hbm_peak": nbytes / (enq[0] * 1e-3) / HBM_PEAK}
            print(f"binary_eval R {R} {kind}: {result[f'binary_eval_{R}_{kind}']}", flush=True)

    if a.no_model:
        with open(a.out, "w") as fh:
            json.dump(result, fh, indent=1, sort_keys=True)
        return
    vocabs = [a.vocab] * a.fields
    model = DeepFM(vocabs, init_std=0.05, device=dev)
    sets = []
    for _ in range(2):
        x = torch.from_numpy(rng.integers(0, a.vocab, (a.val_rows, a.fields))).to(dev)
        y = torch.from_numpy((rng.random(a.val_rows) < 0.4).astype(np.float32)).to(dev)
        sets.append((x, y))

    def torch_evaluate(x, y):
        return torch_eval(torch_logits(model, x, a.batch), y)

    got, ref = model.evaluate(*sets[0], batch_size=a.batch), torch_evaluate(*sets[0])
    nat = time_calls(lambda x, y: model.evaluate(x, y, batch_size=a.batch), sets, a.warmup, a.iters)
    fwd = time_calls(lambda x, y: [model.forward_logits(x[s:s + a.batch]) for s in range(0, a.val_rows, a.batch)],
                     sets, a.warmup, a.iters)
    tor = time_calls(torch_evaluate, sets, a.warmup, a.iters)
    result["evaluate"] = {"native_ms": nat[0], "native_min_ms": nat[1], "native_forward_only_ms": fwd[0],
                          "torch_ms": tor[0], "torch_min_ms": tor[1], "torch_over_native": tor[0] / nat[0],
                          "auc_native": got["AUC"], "auc_torch": ref[0], "logloss_native": got["Logloss"],
                          "logloss_torch": ref[1]}
    print(f"evaluate: {result['evaluate']}", flush=True)

    params = list(model.parameters())
    snapshot = [torch.empty_like(p) for p in params]
    with torch.no_grad():
        snap = time_calls(lambda: torch._foreach_copy_(snapshot, params), [()], a.warmup, a.iters)
    nbytes = sum(p.numel() * 4 for p in params)
    result["snapshot_copy"] = {"ms": snap[0], "min_ms": snap[1], "bytes": nbytes,
                               "gbytes_per_s_read_plus_write": 2 * nbytes / (snap[0] * 1e-3) / 1e9}
    print(f"snapshot copy: {result['snapshot_copy']}", flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
