"""Micro-benchmark of the oblivious-tree boosting path against a plain-PyTorch restatement of the same
model on the same GPU (histograms by index_add_ on int64, scores by cumsum, the first maximum by a masked
min over indices, prediction by gathers; integer sums, so it builds the same trees):

  fit      ObliviousBoostingClassifier.fit at --fit-rows x 12 columns (7 numeric, 5 categorical) and
           --trees trees of depth 6: the reference's CatBoost settings at HMLogImporter's default limit
           (100,000 positives at 1:5). Host clock around the whole call, ending in a synchronise: borders,
           binning, the label read and every tree. The PyTorch restatement runs --torch-trees trees from the
           same bins (its cost per tree does not depend on the tree index) and is compared per tree.
  stages   the kernels one by one at --fit-rows: gradients, the histogram at 1 .. 32 leaves, the split
           search and the leaf update (device events, median).
  predict  ops.gbdt_predict at --predict-rows rows (4096 queries x 100 candidates) under the fitted model.

--loss QuerySoftMax --group-size N times the listwise objective instead (rank_main): the grouped gradient
stage against its PyTorch restatement and one grouped tree against a Logloss tree, at --fit-rows rows in
groups of N; it writes profiles/gbdt_rank_micro_gN.json.

Before timing, the two forms' first trees are compared (the splits exactly, the leaf values to fp32
rounding) and their predictions within fp32 summation error. Writes --out (profiles/gbdt_micro.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_amd  # noqa: E402,F401
from recsys_amd import ops  # noqa: E402
from recsys_amd.temp_model.oblivious_gbdt import ObliviousBoostingClassifier, ObliviousBoostingRanker  # noqa: E402

CARDS = (4, 3, 40, 12, 5)
INV = 1.0 / ops.GBDT_SCALE


def make_rows(R, seed, dev):
    """The tests' generator (tests/gbdt_ref.make) drawn on the device: (num fp32 [R, 7], cat int64 [R, 5], y)."""
    gen = torch.Generator(device=dev).manual_seed(seed)
    num = torch.randn(R, 7, device=dev, generator=gen)
    num[:, 3] = torch.round(num[:, 3] * 2) / 2
    num[:, 6] = num[:, 0]
    cat = torch.stack([torch.randint(0, c, (R,), device=dev, generator=gen) for c in CARDS], dim=1)
    eff = 0.8 * torch.randn(40, device=dev, generator=torch.Generator(device=dev).manual_seed(91))
    z = 1.2 * num[:, 0] - 0.8 * (num[:, 1] > 0.3) + 0.6 * num[:, 2] * (cat[:, 0] == 2) + eff[cat[:, 2]] - 1.6
    y = (torch.rand(R, device=dev, generator=gen) < torch.sigmoid(z)).float()
    return num, cat, y


def torch_tree(bins, y, Fx, is_cat, n_bins, depth, lr, l2):
    """One tree of the model in PyTorch ops, no host read: returns (splits int64 [depth, 2], values fp32 [64])
    and updates Fx in place. bins int64 [F, R]."""
    F, R = bins.shape
    dev = bins.device
    p = (1.0 / (1.0 + torch.exp(-Fx.double()))).float()
    qg = torch.round((y - p).double() * ops.GBDT_SCALE).long()
    qh = torch.round((p * (1.0 - p)).double() * ops.GBDT_SCALE).long()
    leaf = torch.zeros(R, device=dev, dtype=torch.int64)
    feat = torch.arange(F, device=dev)[:, None]
    cand = torch.arange(F * 256, device=dev)
    valid = (torch.arange(256, device=dev)[None, :] < n_bins[:, None])
    splits = []
    for d in range(depth):
        NL = 1 << d
        cell = ((leaf[None, :] * F + feat) * 256 + bins).reshape(-1)
        S = 0.0
        sides = []
        for q in (qg, qh):
            H = torch.zeros(NL * F * 256, device=dev, dtype=torch.int64).index_add_(0, cell, q.expand(F, R).reshape(-1))
            H = H.view(NL, F, 256)
            tot = H.sum(-1, keepdim=True)
            right = torch.where(is_cat[None, :, None], H, tot - torch.cumsum(H, -1))
            sides.append((tot - right, right))
        for side in (0, 1):
            g, h = sides[0][side].double() * INV, sides[1][side].double() * INV
            S = S + g * g / (h + l2)
        S = torch.where(valid, S.sum(0), torch.full((), float("-inf"), device=dev, dtype=torch.float64)).reshape(-1)
        k = torch.where(S == S.max(), cand, torch.full_like(cand, F * 256)).min()      # the first maximum
        f, b = k // 256, k % 256
        col = bins.index_select(0, f.view(1))[0]
        leaf = 2 * leaf + torch.where(is_cat[f], col == b, col > b)
        splits.append(torch.stack([f, b]))
    G = torch.zeros(64, device=dev, dtype=torch.int64).index_add_(0, leaf, qg)
    Hh = torch.zeros(64, device=dev, dtype=torch.int64).index_add_(0, leaf, qh)
    values = (lr * (G.double() * INV / (Hh.double() * INV + l2))).float()
    Fx += values[leaf]
    return torch.stack(splits), values


def torch_predict(bins_u8, f0, splits, values, is_cat, chunk=32):
    """f0 + the trees' leaf values by gathers, `chunk` trees at a time. splits int64 [T, 6, 2]."""
    R = bins_u8.shape[1]
    acc = torch.full((R,), f0, device=bins_u8.device, dtype=torch.float32)
    shift = torch.tensor([32, 16, 8, 4, 2, 1], device=bins_u8.device)[None, :, None]
    for s in range(0, splits.shape[0], chunk):
        f, b = splits[s:s + chunk, :, 0], splits[s:s + chunk, :, 1]
        sel = bins_u8[f]                                                     # [chunk, 6, R]
        right = torch.where(is_cat[f][:, :, None], sel == b[:, :, None], sel > b[:, :, None])
        leaf = (right * shift).sum(1)                                        # [chunk, R]
        acc = acc + values[s:s + chunk].gather(1, leaf).sum(0)
    return acc


def events_ms(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms)


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def torch_grad_query_softmax(Fx, y, row_group, G):
    """The QuerySoftMax gradients in PyTorch ops, no host read: scatter_reduce(amax), exp, index_add_ (a
    float64 sum where the kernel has an int64 one). Returns (qg, qh) int32."""
    rg = row_group.long()
    m = torch.full((G,), float("-inf"), device=Fx.device).scatter_reduce(0, rg, Fx, "amax")
    e = torch.exp(Fx.double() - m[rg].double())
    Z = torch.zeros(G, device=Fx.device, dtype=torch.float64).index_add_(0, rg, e)
    S = torch.zeros(G, device=Fx.device).index_add_(0, rg, y)
    p = (e / Z[rg]).float()
    live = S[rg] > 0
    t = torch.where(y == 1, (1.0 / S.clamp(min=1.0))[rg], torch.zeros_like(y))
    g = torch.where(live, t - p, torch.zeros_like(p))
    h = torch.where(live, p * (1.0 - p), torch.zeros_like(p))
    return (torch.round(g.double() * ops.GBDT_SCALE).int(), torch.round(h.double() * ops.GBDT_SCALE).int())


def rank_main(a):
    """--loss QuerySoftMax: the gradient stage (native against the PyTorch restatement) and one grouped tree
    (against a Logloss tree of the same build) at --fit-rows rows in groups of --group-size, the two forms
    alternating --repeats times (device events, the median of --iters calls each time)."""
    dev = torch.device("cuda", 0)
    R, F, depth, lr, l2 = a.fit_rows, 12, 6, 0.05, 3.0
    num, cat, y = make_rows(R, 1, dev)
    gid = (torch.randperm(R, device=dev, generator=torch.Generator(device=dev).manual_seed(5)) // a.group_size)
    rk = ObliviousBoostingRanker(iterations=a.check_trees, device=dev).fit((num, cat), y, gid)
    plan, model = rk.group_plan_, rk.model_
    bins = rk._bins((num, cat)).index_select(1, plan.order).contiguous()
    yg = y.index_select(0, plan.order).contiguous()
    Fx = ops.gbdt_predict(bins, model)
    qg, qh = ops.gbdt_grad_query_softmax(Fx, yg, plan)
    tg, th = torch_grad_query_softmax(Fx, yg, plan.row_group, plan.G)
    err = max(int((qg - tg).abs().max()), int((qh - th).abs().max())) / ops.GBDT_SCALE
    assert err <= 2e-6, err
    result = {"device": torch.cuda.get_device_name(0), "fit_rows": R, "columns": F, "depth": depth, "group_size": a.group_size,
              "groups": plan.G, "iters": a.iters, "repeats": a.repeats, "max_abs_difference_to_torch": err,
              "kernels_per_grouped_tree": 4 + 4 * depth, "fills_per_grouped_tree": 2 + depth}
    scratch = ops.GBDTScratch(R, F, depth, dev)
    sp, lv = model.splits[0].clone(), model.leaf_values[0].clone()
    forms = {
        "grad_native": lambda: ops.gbdt_grad_query_softmax(Fx, yg, plan, out=(qg, qh)),
        "grad_torch": lambda: torch_grad_query_softmax(Fx, yg, plan.row_group, plan.G),
        "grad_logloss": lambda: ops.gbdt_grad(Fx, yg, out=(qg, qh)),
        "tree_grouped": lambda: ops.gbdt_tree(bins, yg, Fx.clone(), model.is_cat, rk.n_bins_, depth, lr, l2, sp, lv, scratch,
                                              groups=plan),
        "tree_logloss": lambda: ops.gbdt_tree(bins, yg, Fx.clone(), model.is_cat, rk.n_bins_, depth, lr, l2, sp, lv, scratch),
    }
    runs = {name: [] for name in forms}
    for _ in range(a.repeats):
        for name, fn in forms.items():
            runs[name].append(events_ms(fn, 3, a.iters)[0])
    ops._GBDT_GUARD.check()
    result["ms_all"] = runs
    result["ms"] = {name: statistics.median(v) for name, v in runs.items()}
    result["torch_over_native_grad"] = result["ms"]["grad_torch"] / result["ms"]["grad_native"]
    print("QuerySoftMax:", result, flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--loss", choices=("Logloss", "QuerySoftMax"), default="Logloss")
    ap.add_argument("--group-size", type=int, default=6)
    ap.add_argument("--fit-rows", type=int, default=600_000)
    ap.add_argument("--predict-rows", type=int, default=409_600)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--torch-trees", type=int, default=100)
    ap.add_argument("--check-trees", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.loss == "QuerySoftMax":
        a.out = a.out or os.path.join("profiles", f"gbdt_rank_micro_g{a.group_size}.json")
        return rank_main(a)
    a.out = a.out or os.path.join("profiles", "gbdt_micro.json")
    dev = torch.device("cuda", 0)
    num, cat, y = make_rows(a.fit_rows, 1, dev)
    R, F, depth, lr, l2 = a.fit_rows, 12, 6, 0.05, 3.0
    result = {"device": torch.cuda.get_device_name(0), "fit_rows": R, "columns": F, "trees": a.trees, "depth": depth,
              "torch_trees": a.torch_trees, "predict_rows": a.predict_rows, "iters": a.iters, "repeats": a.repeats,
              "kernels_per_tree": 2 + 4 * depth, "fills_per_tree": 1 + depth}

    # the two forms build the same trees
    clf = ObliviousBoostingClassifier(iterations=a.check_trees, device=dev).fit((num, cat), y)
    bins_u8 = clf._bins((num, cat))
    bins = bins_u8.long()
    is_cat, n_bins = clf.model_.is_cat.bool(), clf.n_bins_.long()
    Fx = torch.full((R,), clf.model_.f0, device=dev)
    for t in range(a.check_trees):
        sp, val = torch_tree(bins, y, Fx, is_cat, n_bins, depth, lr, l2)
        assert torch.equal(sp.int(), clf.model_.splits[t]), (t, sp, clf.model_.splits[t])
        # the values to fp32 rounding: the two exp implementations may round one row's sigmoid differently
        assert torch.allclose(val, clf.model_.leaf_values[t], rtol=1e-5, atol=1e-9), t
    assert torch.allclose(Fx, clf.predict_logits((num, cat)), rtol=0, atol=1e-5)
    result["trees_compared"] = a.check_trees

    # fit: the two forms alternate
    fit_ms, torch_ms = [], []
    for _ in range(a.repeats + 1):          # the first round warms both up
        ms, clf = wall_ms(lambda: ObliviousBoostingClassifier(iterations=a.trees, device=dev).fit((num, cat), y))
        fit_ms.append(ms)

        def torch_fit():
            Fx = torch.full((R,), clf.model_.f0, device=dev)
            for _ in range(a.torch_trees):
                torch_tree(bins, y, Fx, is_cat, n_bins, depth, lr, l2)
        torch_ms.append(wall_ms(torch_fit)[0])
    fit_ms, torch_ms = fit_ms[1:], torch_ms[1:]
    nat_tree, tor_tree = statistics.median(fit_ms) / a.trees, statistics.median(torch_ms) / a.torch_trees
    result["fit"] = {"native_ms": statistics.median(fit_ms), "native_ms_all": fit_ms, "native_ms_per_tree": nat_tree,
                     "torch_ms_all": torch_ms, "torch_ms_per_tree": tor_tree, "torch_over_native_per_tree": tor_tree / nat_tree,
                     "torch_ms_extrapolated_to_trees": tor_tree * a.trees}
    print("fit:", result["fit"], flush=True)

    # the stages one by one
    model = clf.model_
    scratch = ops.GBDTScratch(R, F, depth, dev)
    Fx = torch.full((R,), model.f0, device=dev)
    qg, qh = ops.gbdt_grad(Fx, y)
    stages = {"grad": events_ms(lambda: ops.gbdt_grad(Fx, y, out=(qg, qh)), 3, a.iters)[0]}
    gen = torch.Generator(device=dev).manual_seed(3)
    for NL in (1, 2, 4, 8, 16, 32):
        leaf = torch.randint(0, NL, (R,), device=dev, generator=gen).to(torch.uint8)
        hist = torch.empty(NL, F, 256, 2, device=dev, dtype=torch.int64)
        stages[f"histogram_{NL}"] = events_ms(lambda: ops.gbdt_histogram(bins_u8, leaf, qg, qh, NL, out=hist), 3, a.iters)[0]
        stages[f"best_split_{NL}"] = events_ms(lambda: ops.gbdt_best_split(hist, model.is_cat, clf.n_bins_, l2), 3, a.iters)[0]
    split = torch.tensor([0, 100], device=dev, dtype=torch.int32)
    leaf = torch.zeros(R, device=dev, dtype=torch.uint8)

    def apply():
        leaf.zero_()
        ops.gbdt_apply_split(bins_u8, leaf, split, model.is_cat, 16)
    stages["apply_split_with_fill"] = events_ms(apply, 3, a.iters)[0]
    stages["tree"] = events_ms(lambda: ops.gbdt_tree(bins_u8, y, Fx, model.is_cat, clf.n_bins_, depth, lr, l2,
                                                     model.splits[0].clone(), model.leaf_values[0].clone(), scratch), 3,
                               a.iters)[0]
    ops._GBDT_GUARD.check()
    result["stages_ms"] = stages
    print("stages:", stages, flush=True)

    # predict
    pn, pc, _ = make_rows(a.predict_rows, 2, dev)
    pb = clf._bins((pn, pc))
    got = ops.gbdt_predict(pb, model)
    ref = torch_predict(pb, model.f0, model.splits[:model.n_trees].long(), model.leaf_values, is_cat)
    bound = abs(model.f0) + float(model.leaf_values[:model.n_trees].abs().max(1).values.sum())
    err = float((got.double() - ref.double()).abs().max())
    assert err <= 2 * model.n_trees * 2.0 ** -23 * bound, (err, bound)
    nat = events_ms(lambda: ops.gbdt_predict(pb, model), 3, a.iters)
    binning = events_ms(lambda: clf._bins((pn, pc)), 3, a.iters)
    tor = events_ms(lambda: torch_predict(pb, model.f0, model.splits[:model.n_trees].long(), model.leaf_values, is_cat),
                    2, max(3, a.iters // 4))
    result["predict"] = {"trees": model.n_trees, "native_ms": nat[0], "native_min_ms": nat[1], "binning_ms": binning[0],
                         "torch_ms": tor[0], "torch_min_ms": tor[1], "torch_over_native": tor[0] / nat[0],
                         "max_abs_difference": err,
                         "rows_times_trees_per_s": a.predict_rows * model.n_trees / (nat[0] * 1e-3)}
    print("predict:", result["predict"], flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
