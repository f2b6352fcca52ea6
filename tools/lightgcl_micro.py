"""Micro-benchmark of LightGCL's graph propagation and training step on a seeded synthetic bipartite
graph at the reference's scale (1.36M users, 105k items, ~11.3M distinct edges: the reference log's
1375 batches of 8192), Zipf item popularity, D = 64, 2 layers, q = 5, batch 8192.

  * rsx_spmm_norm (one Horner step, Y = E + A^ X) by HIP events, alternating in one loop with
    torch.sparse.mm on the reference's coalesced COO tensor of the same graph on the same device
    (recorded as unavailable if this torch build cannot run it there);
  * bytes from the shape model below against the ~6.3 TB/s achievable HBM rate:
        per stored entry  4 B column index + one D*4-B neighbour row
        per row           D*4 B residual read + D*4 B written
    Half of the entries are in user rows and gather ITEM rows (a 27-MB table at D = 64: it stays in the
    Infinity Cache), half are in item rows and gather USER rows (a 348-MB table: HBM); the model counts
    both at full size, so the item-table half is an upper bound on HBM traffic;
  * LightGCL.train_step against a plain-PyTorch restatement of the reference step written here
    (two torch.sparse.mm, the four dense matmuls with the SVD factors, stack / mean, the losses on the
    full views, torch.optim.Adam), fp32 on both sides, alternating.
Medians with min / max over the timed calls. Writes --out (profiles/lightgcl_micro.json).
--only-step: just the native steps (for rocprofv3 --kernel-trace --stats)."""
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
from recsys_amd.gnn_model import v1_lightgcl as G  # noqa: E402

HBM_BYTES_PER_S = 6.3e12


def synth_edges(num_users, num_items, draws, zipf, seed):
    rng = np.random.default_rng(seed)
    p = 1.0 / np.arange(1, num_items + 1) ** zipf
    items = rng.choice(num_items, size=draws, p=p / p.sum())
    users = rng.integers(0, num_users, draws)
    return torch.from_numpy(np.stack([users, items]).astype(np.int64))


def model_bytes(adj, D, residual=True):
    return adj.nnz * (4 + D * 4) + adj.n * D * 4 * (2 if residual else 1)


class TorchLightGCL(nn.Module):
    """The reference step's arithmetic in plain PyTorch (fp32, no AMP)."""

    def __init__(self, src, coo):
        super().__init__()
        self.nu, self.L, self.temp = src.num_users, src.n_layers, src.temp
        self.coo, self.U, self.S, self.V = coo, src.U, src.S, src.V
        self.embedding_user = nn.Embedding.from_pretrained(src.embedding_user.weight.detach().clone(), freeze=False)
        self.embedding_item = nn.Embedding.from_pretrained(src.embedding_item.weight.detach().clone(), freeze=False)

    def forward(self):
        e = torch.cat([self.embedding_user.weight, self.embedding_item.weight])
        loc, x = [e], e
        for _ in range(self.L):
            x = torch.sparse.mm(self.coo, x)
            loc.append(x)
        glo, x = [e], e
        for _ in range(self.L):
            x = torch.matmul(self.U, torch.matmul(self.V.t(), x) * self.S.unsqueeze(1))
            glo.append(x)
        return torch.mean(torch.stack(loc, 1), 1), torch.mean(torch.stack(glo, 1), 1)

    def loss(self, users, pos, neg, lambda_ssl, lambda_reg):
        loc, glo = self()
        ue, pe, ne = loc[users], loc[pos + self.nu], loc[neg + self.nu]
        bpr = -torch.mean(torch.log(torch.sigmoid((ue * pe).sum(1) - (ue * ne).sum(1)) + 1e-10))
        ln, gn = F.normalize(loc, dim=1), F.normalize(glo, dim=1)
        ssl = 0.0
        for idx in (torch.unique(users), torch.unique(pos + self.nu)):
            logits = torch.clamp(ln[idx] @ gn[idx].t() / self.temp, max=100.0)
            ssl = ssl + F.cross_entropy(logits, torch.arange(idx.numel(), device=idx.device))
        reg = 0.5 * (self.embedding_user.weight[users].norm(2).pow(2) + self.embedding_item.weight[pos].norm(2).pow(2)
                     + self.embedding_item.weight[neg].norm(2).pow(2))
        return bpr + lambda_ssl * ssl + lambda_reg * reg


def timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--users", type=int, default=1_360_000)
    ap.add_argument("--items", type=int, default=105_000)
    ap.add_argument("--draws", type=int, default=11_280_000, help="edge draws before duplicates are removed")
    ap.add_argument("--zipf", type=float, default=0.7)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--batch", type=int, default=8192)
    ap.add_argument("--iters", type=int, default=20, help="timed native steps")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--torch-iters", type=int, default=8, help="timed plain-PyTorch steps")
    ap.add_argument("--spmm-iters", type=int, default=50, help="timed calls of each SpMM")
    ap.add_argument("--only-step", action="store_true")
    ap.add_argument("--out", default=os.path.join("profiles", "lightgcl_micro.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    cfg = {"emb_dim": a.dim, "n_layers": 2, "temp": 0.2, "lambda_ssl": 0.01, "lambda_reg": 1e-5}
    edges = synth_edges(a.users, a.items, a.draws, a.zipf, seed=0)
    adj = G.NormAdjacency(edges, a.users, a.items, device=dev)
    deg = adj.row_ptr[1:] - adj.row_ptr[:-1]
    result = {"users": a.users, "items": a.items, "edges": adj.nnz // 2, "nnz": adj.nnz, "dim": a.dim,
              "batch": a.batch, "device": torch.cuda.get_device_name(0), "zipf": a.zipf,
              "max_item_degree": int(deg[a.users:].max()), "max_user_degree": int(deg[:a.users].max()),
              "long_rows": adj.long_rows.numel(), "chunks": adj.chunk_beg.numel(),
              "edges_in_long_rows": int(deg[adj.long_rows].sum()), "chunk_len": ops.SPMM_CHUNK}
    print(json.dumps(result), flush=True)
    coo = None
    try:
        coo = adj.to_sparse_coo()
        U, S, V = torch.svd_lowrank(coo, q=5, niter=2)
        result["svd"] = "torch.svd_lowrank on the device"
    except Exception as exc:  # the timings do not depend on the factors' values
        g = torch.Generator().manual_seed(1)
        U = torch.linalg.qr(torch.randn(adj.n, 5, generator=g))[0].to(dev)
        V, S = U.clone(), torch.linspace(1.0, 0.5, 5, device=dev)
        result["svd"] = f"orthonormal stand-in factors (svd_lowrank failed: {type(exc).__name__}: {exc})"[:300]
    torch.manual_seed(0)
    model = G.LightGCL(a.users, a.items, cfg, adj, (U, S, V)).to(dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    g = torch.Generator().manual_seed(2)

    def batch():
        idx = torch.randint(0, edges.shape[1], (a.batch,), generator=g)
        return (edges[0, idx].to(dev), edges[1, idx].to(dev),
                torch.randint(0, a.items, (a.batch,), generator=g).to(dev))

    data = [batch() for _ in range(4)]
    if a.only_step:
        for i in range(a.warmup + a.iters):
            model.train_step(*data[i % 4], opt)
        torch.cuda.synchronize()
        return

    # one propagation hop, ours against torch.sparse.mm, alternating
    X = torch.randn(adj.n, a.dim, device=dev)
    E = torch.randn(adj.n, a.dim, device=dev)
    out = torch.empty_like(X)
    ours, theirs, sparse_err = [], [], None
    for i in range(a.warmup + a.spmm_iters):
        t = timed_ms(lambda: ops.spmm_norm(adj, X, R=E, out=out))
        if i >= a.warmup:
            ours.append(t)
        if coo is not None and sparse_err is None:
            try:
                t = timed_ms(lambda: torch.sparse.mm(coo, X))
                if i >= a.warmup:
                    theirs.append(t)
            except Exception as exc:
                sparse_err = f"{type(exc).__name__}: {exc}"[:300]
    nb = model_bytes(adj, a.dim)
    result["spmm_norm"] = dict(summary(ours), model_bytes=nb,
                               gbytes_per_s=nb / (statistics.median(ours) * 1e-3) / 1e9,
                               fraction_of_hbm=nb / (statistics.median(ours) * 1e-3) / HBM_BYTES_PER_S,
                               gather_bytes_from_item_table=adj.nnz // 2 * a.dim * 4,
                               gather_bytes_from_user_table=adj.nnz // 2 * a.dim * 4,
                               item_table_bytes=a.items * a.dim * 4, user_table_bytes=a.users * a.dim * 4)
    if theirs:
        result["torch_sparse_mm"] = dict(summary(theirs), note="A^ X alone (no residual add)")
        result["spmm_speedup_over_torch"] = statistics.median(theirs) / statistics.median(ours)
        ref = torch.sparse.mm(coo, X) + E
        result["spmm_max_abs_diff_vs_torch"] = float((ops.spmm_norm(adj, X, R=E) - ref).abs().max())
        del ref
    else:
        result["torch_sparse_mm"] = {"unavailable": sparse_err or "no COO tensor on the device"}
    print(json.dumps({k: result[k] for k in ("spmm_norm", "torch_sparse_mm")}), flush=True)

    # the training step, ours against the plain-PyTorch restatement, alternating
    ref_model, ref_err = None, None
    if coo is not None and sparse_err is None:
        ref_model = TorchLightGCL(model, coo).to(dev)
        ref_opt = torch.optim.Adam(ref_model.parameters(), lr=1e-3)

    def torch_step(users, pos, neg):
        ref_opt.zero_grad()
        ref_model.loss(users, pos, neg, cfg["lambda_ssl"], cfg["lambda_reg"]).backward()
        ref_opt.step()

    ours, theirs = [], []
    for i in range(a.warmup + a.iters):
        t = timed_ms(lambda: model.train_step(*data[i % 4], opt))
        if i >= a.warmup:
            ours.append(t)
        if ref_model is not None and ref_err is None and i < a.warmup + a.torch_iters:
            try:
                t = timed_ms(lambda: torch_step(*data[i % 4]))
                if i >= a.warmup:
                    theirs.append(t)
            except Exception as exc:
                ref_err = f"{type(exc).__name__}: {exc}"[:300]
    ops.timing_start()
    for i in range(3):
        model.train_step(*data[i % 4], opt)
    result["train_step"] = dict(summary(ours), phase_ms={k: v[1] / 3 for k, v in ops.timing_stop().items()})
    if theirs:
        result["torch_step"] = summary(theirs)
        result["step_speedup_over_torch"] = statistics.median(theirs) / statistics.median(ours)
    else:
        result["torch_step"] = {"unavailable": ref_err or sparse_err or "no COO tensor on the device"}
    print(json.dumps({k: result[k] for k in ("train_step", "torch_step")}), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
