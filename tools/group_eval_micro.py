"""Micro-benchmark of the grouped evaluation: ops.group_eval at R = 65,536 and 1,048,576 with groups
of 6 (the importer's 1 positive + 5 negatives), groups of 100 (rerank top-100) and one group over
everything, against the same computation in plain PyTorch on the same GPU (two stable sorts, cummax /
cumsum for the heads and counts, index_add_ per group; its DCG sum uses float atomics). Before timing,
the two forms' per-group P, N and U2 are compared exactly and their means loosely. Every timed call
ends with its one host read. Event timing, warm-up first, median over --iters calls on fresh inputs
in rotation. Also the achieved bytes/s against DESIGN.md's byte model. Writes --out
(profiles/group_eval_micro.json)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_amd  # noqa: E402,F401
from recsys_amd import ops  # noqa: E402

HBM_PEAK = 8e12   # bytes/s
TOP = 10


def eval_bytes(R, G, key_bits):
    """DESIGN.md's byte model of one rsx_group_eval on the radix-pass side of the sort: the key pass
    reads logit, y and the group id (12 B a row) and writes key + label (9 B); the sort reads the keys
    once for its histograms (8 B) and moves the 9-B pairs in and out in each 8-bit digit pass (18 B a
    pass); the two tile passes read the sorted pairs (9 B each); the per-group rows (36 B) are written
    once and read once."""
    passes = (key_bits + 7) // 8
    return R * (12 + 9 + 8 + 18 * passes + 9 + 9) + G * 72


def torch_group_eval(z, y, g, D, top):
    """The same per-group integers and the two means in plain PyTorch. Returns (the summary dict, the
    per-group tensors P, N, U2 sized R with the first G entries in use)."""
    R = z.numel()
    o1 = torch.argsort(-z, stable=True)
    idx = o1[torch.argsort(g[o1], stable=True)]
    zs, ys, gs = z[idx], y[idx].to(torch.int64), g[idx]
    rows = torch.arange(R, device=z.device)
    one = torch.ones(1, device=z.device, dtype=torch.bool)
    ghead = torch.cat([one, gs[1:] != gs[:-1]])
    thead = ghead | torch.cat([one, zs[1:] != zs[:-1]])
    ttail = torch.cat([thead[1:], one])
    gord = torch.cumsum(ghead, 0) - 1
    gstart = torch.cummax(torch.where(ghead, rows, 0), 0)[0]
    tstart = torch.cummax(torch.where(thead, rows, 0), 0)[0]
    neg = 1 - ys
    cn = torch.cumsum(neg, 0)
    cx = cn - neg
    length = rows - tstart + 1
    pos = torch.where(ttail, length - (cn - cx[tstart]), 0)
    v = pos * ((cx[tstart] - cx[gstart]) + (cn - cx[gstart]))
    d = pos.double() * (D[(rows + 1 - gstart).clamp(max=top)] - D[(tstart - gstart).clamp(max=top)]) / length.double()
    zero = torch.zeros(R, device=z.device, dtype=torch.int64)
    P, Nn, V = zero.index_add(0, gord, ys), zero.index_add(0, gord, neg), zero.index_add(0, gord, v)
    dcg = torch.zeros(R, device=z.device, dtype=torch.float64).index_add(0, gord, d)
    U2 = 2 * P * Nn - V
    has_p, both = P > 0, (P > 0) & (Nn > 0)
    ndcg = torch.where(has_p, dcg / D[P.clamp(max=top)].clamp(min=1.0), 0.0)
    auc = torch.where(both, U2.double() / (2 * P * Nn).clamp(min=1).double(), 0.0)
    s = torch.stack([(gord[-1] + 1).double(), has_p.sum().double(), both.sum().double(), ndcg.sum(), auc.sum()]).tolist()
    G, ng, na = int(s[0]), int(s[1]), int(s[2])
    return ({"ndcg": s[3] / ng if ng else float("nan"), "query_auc": s[4] / na if na else float("nan"), "groups": G,
             "ndcg_groups": ng, "auc_groups": na}, (P, Nn, U2))


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
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "group_eval_micro.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(5)
    D = ops.ndcg_discounts(TOP, dev)
    result = {"iters": a.iters, "warmup": a.warmup, "device": torch.cuda.get_device_name(0), "top": TOP,
              "hbm_peak_bytes_per_s": HBM_PEAK}
    for R in a.rows:
        for kind, size in (("groups_of_6", 6), ("groups_of_100", 100), ("one_group", R)):
            inputs = []
            for _ in range(8):
                z = np.round(rng.standard_normal(R), 2).astype(np.float32)        # ties occur
                y = (rng.random(R) < (1 / 6 if size == 6 else 0.1)).astype(np.float32)
                g = rng.permutation(R) // size
                inputs.append(tuple(torch.from_numpy(t).to(dev) for t in (z, y, g)))
            gmax = (R - 1) // size
            ref, (P, Nn, U2) = torch_group_eval(*inputs[0], D, TOP)
            got = ops.group_eval(*inputs[0], top=TOP)
            res = got.result()
            G = res["groups"]
            _, gP, gN, gU2, _ = got.per_group()
            assert all(res[k] == ref[k] for k in ("groups", "ndcg_groups", "auc_groups")), (res, ref)
            assert torch.equal(gP, P[:G]) and torch.equal(gN, Nn[:G]) and torch.equal(gU2, U2[:G])
            assert abs(res["ndcg"] - ref["ndcg"]) < 1e-9 and abs(res["query_auc"] - ref["query_auc"]) < 1e-9, (res, ref)
            nat = time_calls(lambda z, y, g: ops.group_eval(z, y, g, top=TOP).result(), inputs, a.warmup, a.iters)
            bnd = time_calls(lambda z, y, g: ops.group_eval(z, y, g, top=TOP, max_group_id=gmax).result(), inputs,
                             a.warmup, a.iters)
            enq = time_calls(lambda z, y, g: ops.group_eval(z, y, g, top=TOP), inputs, a.warmup, a.iters)
            tor = time_calls(lambda z, y, g: torch_group_eval(z, y, g, D, TOP), inputs, a.warmup, a.iters)
            nbytes = eval_bytes(R, G, 63)
            result[f"group_eval_{R}_{kind}"] = {
                "groups": G, "native_ms": nat[0], "native_min_ms": nat[1], "native_max_group_id_ms": bnd[0],
                "native_without_read_ms": enq[0], "torch_ms": tor[0], "torch_min_ms": tor[1],
                "torch_over_native": tor[0] / nat[0], "model_bytes": nbytes,
                "model_bytes_max_group_id": eval_bytes(R, G, 32 + max(gmax, 1).bit_length()),
                "gbytes_per_s": nbytes / (enq[0] * 1e-3) / 1e9, "fraction_of_hbm_peak": nbytes / (enq[0] * 1e-3) / HBM_PEAK,
                "ndcg": res["ndcg"], "query_auc": res["query_auc"]}
            print(f"group_eval R {R} {kind}: {result[f'group_eval_{R}_{kind}']}", flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
