"""Micro-benchmark of the ensemble evaluation's device stages (tower_code/mined_inference.py) on one batch
of users: seeded unit vectors, 64-wide GNN space, 128-wide sequence space.

  * pool: both retrievers' pools of 1000, as the evaluators form them (per chunk of users bounded to
    512 MB of scores: fp32 torch.matmul, then ops.select_topk_rows), beside the same chunks with
    torch.topk, and the pools from ops.retrieve_topk ("fused": the bf16 scan with exact rescoring where
    its plan serves the corpus, one corpus image built per retriever and call; "fused_path" tells which
    route the op took); and the selection alone on one resident chunk of scores beside torch.topk on it;
  * fuse: ops.fuse_rank over the joined pool of 2000 with 11 alphas, min-max and RRF, beside a
    plain-PyTorch restatement of the same batch kept on the device (gather, both score sets,
    normalisation or double-argsort ranks, per alpha the weighted sum, torch.topk(max_k + 20), first
    occurrences by a stable sort, hit@k against a padded truth). The reference's own form adds a
    device-to-host copy per alpha and Python loops over the users; that part is not timed;
  * k = 512, 1000, 2048: torch.matmul + ops.select_topk_rows beside ops.retrieve_topk (the scan fused with
    the dot products where its plan serves the corpus), 128-wide, with the fused path's fallback count.
--stages pool runs the pool stage alone (the evaluators' switch between the two forms,
profiles/ensemble_pool_switch.json).
Every side runs on the same GPU in the same process, alternating after warm-up, each call between HIP
events; medians with min / max. Writes --out (profiles/ensemble_micro.json)."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_amd  # noqa: E402,F401
from recsys_amd import ops  # noqa: E402
from recsys_amd.tower_code import mined_inference as MI  # noqa: E402

K_LIST = [20, 100, 500]
POOL = 1000
TRUTH_PAD = 8


def unit(n, d, generator, device):
    return F.normalize(torch.randn(n, d, generator=generator), dim=1).to(device)


def timed_ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1), out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "calls": len(ms)}


def alternate(sides, warmup, iters):
    """{name: summary} of the callables in `sides`, called in turn."""
    ms = {k: [] for k in sides}
    for i in range(warmup + iters):
        for k, fn in sides.items():
            t, _ = timed_ms(fn)
            if i >= warmup:
                ms[k].append(t)
    return {k: summary(v) for k, v in ms.items()}


def pools(u, items, k, step, select):
    out = []
    for s in range(0, u.shape[0], step):
        out.append(select(torch.matmul(u[s:s + step], items.T), k))
    return torch.cat(out)


def torch_fuse(gu, gi, su, si, cand, wa, wb, mode, k_rrf, cut, ks, truth_pad):
    """The reference's per-batch body (:1115-1189 / :1336-1410) in plain PyTorch, kept on the device."""
    B, C = cand.shape
    flat = cand.reshape(-1).long()
    s_g = (gu.unsqueeze(1) * gi[flat].view(B, C, -1)).sum(dim=-1)
    s_s = (su.unsqueeze(1) * si[flat].view(B, C, -1)).sum(dim=-1)
    if mode == "minmax":
        def norm(t):
            mn, mx = t.min(dim=1, keepdim=True)[0], t.max(dim=1, keepdim=True)[0]
            return (t - mn) / (mx - mn + 1e-9)
    else:
        ranks = torch.arange(C, device=cand.device, dtype=torch.float32).expand(B, -1)

        def norm(t):
            order = torch.argsort(t, dim=1, descending=True, stable=True)
            return 1.0 / (k_rrf + torch.zeros_like(t).scatter_(1, order, ranks) + 1.0)
    n_g, n_s = norm(s_g), norm(s_s)
    hits = []
    for a, b in zip(wa, wb):
        _, local = torch.topk(a * n_g + b * n_s, k=cut, dim=1)
        ids = torch.gather(cand, 1, local).long()
        sid, order = torch.sort(ids, dim=1, stable=True)              # equal ids keep their order: the run's head is the first seen
        head = torch.ones_like(sid, dtype=torch.bool)
        head[:, 1:] = sid[:, 1:] != sid[:, :-1]
        keep = torch.zeros_like(head).scatter_(1, order, head)
        rank = torch.cumsum(keep, dim=1) - 1
        found = (ids.unsqueeze(-1) == truth_pad.unsqueeze(1)).any(dim=-1) & keep
        first = torch.where(found, rank, torch.full_like(rank, cut)).min(dim=1)[0]
        hits.append(torch.stack([first < k for k in ks], dim=1))
    return torch.stack(hits, dim=1)   # [B, A, nK] bool


def run(n_items, a, dev, g):
    B = a.batch
    gu, su = unit(B, 64, g, dev), unit(B, 128, g, dev)
    gi, si = unit(n_items, 64, g, dev), unit(n_items, 128, g, dev)
    step = MI._chunk_rows(B, n_items)
    iters = a.iters if n_items <= 100_000 else max(3, a.iters // 4)
    res = {"items": n_items, "batch": B, "chunk_rows": step, "pool": POOL}

    sel_ours = lambda S, k: ops.select_topk_rows(S, k)[0]
    sel_torch = lambda S, k: torch.topk(S, k=k, dim=1)[1].to(torch.int32)
    gu128, gi128 = MI._pad128(gu), MI._pad128(gi).contiguous()
    fused = lambda u, items: ops.retrieve_topk(u, items, POOL)[1].to(torch.int32)
    res["pool_both_retrievers"] = alternate({
        "native": lambda: (pools(gu, gi, POOL, step, sel_ours), pools(su, si, POOL, step, sel_ours)),
        "torch": lambda: (pools(gu, gi, POOL, step, sel_torch), pools(su, si, POOL, step, sel_torch)),
        "fused": lambda: (fused(gu128, gi128), fused(su, si)),
    }, a.warmup, iters)
    diag = {}
    ops.retrieve_topk(su, si, POOL, diag=diag)
    res["pool_both_retrievers"]["fused_path"] = diag["path"]
    res["pool_both_retrievers"]["fused_fallback_queries_seq"] = diag["fallback_queries"]
    if a.stages == "pool":
        ops.clear_retrieval_cache()
        return res
    S = torch.matmul(su[:step], si.T)
    res["select_alone_one_chunk"] = dict(alternate({
        "native": lambda: ops.select_topk_rows(S, POOL), "torch": lambda: torch.topk(S, k=POOL, dim=1)}, a.warmup, iters),
        rows=S.shape[0], bytes=S.numel() * 4)
    ours, theirs = ops.select_topk_rows(S, POOL), torch.topk(S, k=POOL, dim=1)
    res["select_values_equal_torch"] = bool(torch.equal(ours[1], theirs[0]))
    del S, ours, theirs

    pool_g, pool_s = pools(gu, gi, POOL, step, sel_ours), pools(su, si, POOL, step, sel_ours)
    cand = torch.cat([pool_g, pool_s], dim=1).contiguous()
    gen = torch.Generator().manual_seed(1)
    # ground truth: up to TRUTH_PAD items per user, one of them from the pool for half of the users
    truth_pad = torch.randint(0, n_items, (B, TRUTH_PAD), generator=gen)
    truth_pad[::2, 0] = cand[::2, 700].cpu().long()
    gt = {u: set(truth_pad[u].tolist()) for u in range(B)}
    off, tr = MI.truth_csr(gt, list(range(B)), n_items)
    off_d, tr_d, truth_pad = torch.from_numpy(off).to(dev), torch.from_numpy(tr).to(dev), truth_pad.to(dev)
    alphas = MI.alpha_grid(0.1)
    wa, wb = MI.fusion_weights(alphas)
    cut = max(K_LIST) + 20
    for mode in ("minmax", "rrf"):
        native = lambda: ops.fuse_rank(gu, gi, su, si, cand, alphas, K_LIST, off_d, tr_d, mode=mode, k_rrf=200.0,
                                       cut=cut).hits
        plain = lambda: torch_fuse(gu, gi, su, si, cand, wa.tolist(), wb.tolist(), mode, 200.0, cut, K_LIST, truth_pad)
        res[f"fuse_{mode}"] = alternate({"native": native, "torch": plain}, a.warmup, iters)
        bits = native()
        ours = torch.stack([(bits >> j) & 1 for j in range(len(K_LIST))], dim=-1).bool()
        res[f"fuse_{mode}"]["users_whose_hits_differ_from_torch"] = int((ours != plain()).any(dim=-1).any(dim=-1).sum())
        res[f"fuse_{mode}"]["hit_rate_at_k_alpha_0.5"] = ours[:, 5].float().mean(dim=0).tolist()

    for k in (512, 1000, 2048):
        res[f"k{k}"] = alternate({
            "matmul_select_topk_rows": lambda: pools(su, si, k, step, sel_ours),
            "retrieve_topk": lambda: ops.retrieve_topk(su, si, k)[1],
        }, a.warmup, iters)
        # the two form the fp32 dot products in different orders, so near-equal scores may swap places
        diag = {}
        differ = (pools(su, si, k, step, sel_ours).long() != ops.retrieve_topk(su, si, k, diag=diag)[1])
        res[f"k{k}"]["places_that_differ"] = int(differ.sum())
        res[f"k{k}"]["places"] = differ.numel()
        res[f"k{k}"]["retrieve_topk_path"] = diag["path"]
        res[f"k{k}"]["fallback_queries"] = diag["fallback_queries"]
    ops.clear_retrieval_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, nargs="+", default=[47_062, 1_000_000])
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--stages", choices=["all", "pool"], default="all")
    ap.add_argument("--out", default=os.path.join("profiles", "ensemble_micro.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "alphas": 11, "k_list": K_LIST, "runs": []}
    with torch.no_grad():
        for n in a.items:
            r = run(n, a, dev, torch.Generator().manual_seed(0))
            print(json.dumps(r), flush=True)
            result["runs"].append(r)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
