"""Micro-benchmark of the DeepFM training step at BASELINE configs[2] (65,536 rows x 39 fields,
d=16, vocab 1e6/field): the native step (DeepFM.make_trainer().step) against the same step in plain
PyTorch on the same GPU (nn.Embedding(sparse=True) lookups, autograd, torch.optim.SparseAdam on the
tables, Adam on the dense parameters), on Zipf(1.1) and on uniform ids. Event timing, warm-up first,
median over --iters steps on fresh batches. Also the native step's phases (ops.timed) and the
achieved bytes/s of its sparse half (contribution rows + coalesce + row update) against the byte
model of DESIGN.md. Writes --out (profiles/deepfm_train_micro.json)."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_amd  # noqa: E402,F401
from recsys_amd import ops  # noqa: E402
from recsys_amd.temp_model.ranker_skelet import DeepFM  # noqa: E402


class TorchDeepFM(nn.Module):
    """The same model with sparse-gradient embeddings, for autograd + SparseAdam."""

    def __init__(self, vocabs, dev):
        super().__init__()
        self.emb = nn.ModuleList([nn.Embedding(v, 16, sparse=True) for v in vocabs])
        self.lin = nn.ModuleList([nn.Embedding(v, 1, sparse=True) for v in vocabs])
        self.l1, self.l2 = nn.Linear(len(vocabs) * 16, 256), nn.Linear(256, 128)
        self.out = nn.Linear(128, 1, bias=False)
        self.bias = nn.Parameter(torch.zeros(1))
        for e in list(self.emb) + list(self.lin):
            nn.init.normal_(e.weight, std=0.05)
        self.to(dev)

    def forward(self, x):
        v = torch.stack([e(x[:, f]) for f, e in enumerate(self.emb)], dim=1)
        first = sum(e(x[:, f]).squeeze(1) for f, e in enumerate(self.lin))
        fm = 0.5 * (v.sum(1) ** 2 - (v * v).sum(1)).sum(1)
        h = F.relu(self.l2(F.relu(self.l1(v.flatten(1)))))
        return self.bias + first + fm + self.out(h).squeeze(1)


def batches(kind, rows, nf, vocab, count, dev, rng):
    out = []
    for _ in range(count):
        if kind == "uniform":
            x = rng.integers(0, vocab, (rows, nf))
        else:
            x = ((rng.zipf(1.1, size=(rows, nf)) - 1) % vocab).astype(np.int64)
        y = (rng.random(rows) < 0.4).astype(np.float32)
        out.append((torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev)))
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


def sparse_bytes(n, distinct):
    """DESIGN.md's byte model of the sparse half: contrib_k reads emb, dE (64 B each) and inv (4 B)
    and stores gV + gW (68 B) per (row, field); the coalescing pass reads the 68 B back; every
    distinct (field, id) reads and writes three 68-B row streams (p, m, v) and reads its key and
    segment bounds (12 B)."""
    return n * (64 + 64 + 4 + 68 + 68) + distinct * (3 * 2 * 68 + 12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--fields", type=int, default=39)
    ap.add_argument("--vocab", type=int, default=1_000_000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join("profiles", "deepfm_train_micro.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    vocabs = [a.vocab] * a.fields
    n = a.rows * a.fields
    rng = np.random.default_rng(3)
    result = {"rows": a.rows, "fields": a.fields, "vocab": a.vocab, "iters": a.iters, "warmup": a.warmup,
              "device": torch.cuda.get_device_name(0)}

    model = DeepFM(vocabs, init_std=0.05, device=dev)
    tr = model.make_trainer(lr=1e-3)
    data = {k: batches(k, a.rows, a.fields, a.vocab, 8, dev, rng) for k in ("zipf", "uniform")}
    for kind in ("zipf", "uniform"):
        med, best = time_steps(tr.step, data[kind], a.warmup, a.iters)
        ops.timing_start()
        for i in range(a.iters):
            tr.step(*data[kind][i % 8])
        phases = {k: v[1] / a.iters for k, v in ops.timing_stop().items() if k.startswith("deepfm_train/")
                  and k.count("/") == 1}
        fld = torch.arange(a.fields, device=dev, dtype=torch.int64) << 40
        distinct = statistics.mean(int(torch.unique(x + fld).numel()) for x, _ in data[kind])
        model_bytes = sparse_bytes(n, distinct)
        sp = phases["deepfm_train/sparse"]
        result[f"native_{kind}"] = {"median_ms": med, "min_ms": best, "phase_ms": phases, "distinct_ids": distinct,
                                    "sparse_model_bytes": model_bytes, "sparse_ms": sp,
                                    "sparse_gbytes_per_s": model_bytes / (sp * 1e-3) / 1e9}
        print(f"native {kind}: median {med:.3f} ms, phases {phases}", flush=True)
    tr.check_ids()
    del tr, model
    torch.cuda.empty_cache()

    ref = TorchDeepFM(vocabs, dev)
    tables = [e.weight for e in list(ref.emb) + list(ref.lin)]
    dense = [p for p in ref.parameters() if not any(p is t for t in tables)]
    so, do = torch.optim.SparseAdam(tables, lr=1e-3), torch.optim.Adam(dense, lr=1e-3)

    def torch_step(x, y):
        so.zero_grad(set_to_none=True)
        do.zero_grad(set_to_none=True)
        loss = F.binary_cross_entropy_with_logits(ref(x), y)
        loss.backward()
        so.step()
        do.step()
        return loss

    for kind in ("zipf", "uniform"):
        med, best = time_steps(torch_step, data[kind], a.warmup, a.iters)
        result[f"torch_{kind}"] = {"median_ms": med, "min_ms": best}
        print(f"torch {kind}: median {med:.3f} ms", flush=True)
    result["zipf_over_uniform"] = result["native_zipf"]["median_ms"] / result["native_uniform"]["median_ms"]
    result["speedup_zipf"] = result["torch_zipf"]["median_ms"] / result["native_zipf"]["median_ms"]
    result["speedup_uniform"] = result["torch_uniform"]["median_ms"] / result["native_uniform"]["median_ms"]
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
    print(json.dumps({k: result[k] for k in ("zipf_over_uniform", "speedup_zipf", "speedup_uniform")}), flush=True)


if __name__ == "__main__":
    main()
