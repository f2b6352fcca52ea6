"""Micro-benchmark of the boosted ranker's explanation kernels (csrc/gbdt_explain.hip) against a plain-PyTorch
restatement on the same GPU, at the README's serving shape: --rows (4096 queries x 100 candidates) x 12 columns
under --trees trees of depth 6 fitted on --fit-rows rows.

  shap          ops.gbdt_shap against gathers of the same table and an fp64 einsum per chunk of --torch-chunk
                trees: the rows' bits, the players' index offsets and the 64 coalition indices by einsum, one
                gather of the table, the Shapley coefficients as a [tree, player, coalition] tensor, index_add_
                into the feature rows.
  explain_plan  ops.gbdt_explain_plan against the same recursion level by level over all trees at once.
  leaf_weights  ops.gbdt_leaf_weights at --rows and at --weight-rows rows against leaf indices by gathers and
                one index_add_ of ones per chunk.

Before timing, the two forms of each are compared: the weights exactly, the table, the level sums and the SHAP
values within the tests' bounds. Device events, the median of --iters calls, the two forms alternating --repeats
times. Writes --out (profiles/gbdt_explain_micro.json)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_amd  # noqa: E402,F401
from recsys_amd import ops  # noqa: E402
from recsys_amd.temp_model.oblivious_gbdt import ObliviousBoostingClassifier  # noqa: E402
from tools.gbdt_micro import events_ms, make_rows  # noqa: E402

DEPTH = 6
P3 = [3 ** (DEPTH - 1 - d) for d in range(DEPTH)]
FULL = 3 ** DEPTH - 1


def shapley_w(s, m):
    from math import factorial
    return factorial(s) * factorial(m - s - 1) / factorial(m)


def torch_bits(bins_u8, splits, is_cat):
    """go right [n, 6, R] (bool) of the trees splits int64 [n, 6, 2]."""
    f, b = splits[:, :, 0], splits[:, :, 1]
    sel = bins_u8[f]
    return torch.where(is_cat[f][:, :, None], sel == b[:, :, None], sel > b[:, :, None])


def torch_leaf_weights(bins_u8, splits, is_cat, chunk=32):
    T, R = splits.shape[0], bins_u8.shape[1]
    shift = torch.tensor([32, 16, 8, 4, 2, 1], device=bins_u8.device)[None, :, None]
    out = torch.zeros(T * 64, device=bins_u8.device, dtype=torch.int64)
    ones = torch.ones(chunk * R, device=bins_u8.device, dtype=torch.int64)
    for s in range(0, T, chunk):
        leaf = (torch_bits(bins_u8, splits[s:s + chunk], is_cat) * shift).sum(1)            # [n, R]
        cell = leaf + 64 * torch.arange(s, s + leaf.shape[0], device=leaf.device)[:, None]
        out.index_add_(0, cell.reshape(-1), ones[:cell.numel()])
    return out.view(T, 64)


def torch_plan(values, weights):
    """(table float64 [T, 729], pvc float64 [T, 6]) of depth-6 trees, every tree at once."""
    T = values.shape[0]
    v, w = values.double(), weights.double()
    cur, cov = v.view(T, 64, 1), w.view(T, 64, 1)
    for _ in range(DEPTH):
        a, b, c0, c1 = cur[:, 0::2], cur[:, 1::2], cov[:, 0::2], cov[:, 1::2]
        live = (c0 + c1) > 0
        mix = torch.where(live, (c0 * a + c1 * b) / torch.where(live, c0 + c1, torch.ones_like(c0)), 0.5 * a + 0.5 * b)
        cur, cov = torch.cat([a, b, mix], dim=2), c0 + c1
    pvc = []
    for d in range(DEPTH):
        shape = (T, 1 << d, 2, 32 >> d)
        c, x = w.view(shape), v.view(shape)
        c1, c2 = c[:, :, 0], c[:, :, 1]
        live = (c1 + c2) > 0
        term = torch.where(live, c1 * c2 / torch.where(live, c1 + c2, torch.ones_like(c1)) * (x[:, :, 0] - x[:, :, 1]) ** 2,
                           torch.zeros_like(c1))
        pvc.append(term.reshape(T, -1).sum(1))
    return cur.view(T, 729), torch.stack(pvc, dim=1)


def shap_structure(splits_host, dev):
    """Per tree, from the splits on the host (once): own float64 [T, 6 players, 6 levels], coef float64 [T, 6
    players, 64 coalitions] (0 for a coalition with a player the tree does not have) and feat int64 [T, 6]."""
    T = splits_host.shape[0]
    own, coef, feat = torch.zeros(T, 6, 6, dtype=torch.float64), torch.zeros(T, 6, 64, dtype=torch.float64), torch.zeros(T, 6, dtype=torch.int64)
    for t in range(T):
        players = []
        for d in range(DEPTH):
            f = int(splits_host[t, d, 0])
            if f not in players:
                players.append(f)
            own[t, players.index(f), d] = 1.0
        m = len(players)
        feat[t, :m] = torch.tensor(players)
        for mask in range(1 << m):
            size = bin(mask).count("1")
            for j in range(m):
                coef[t, j, mask] = shapley_w(size - 1, m) if mask >> j & 1 else -shapley_w(size, m)
    return own.to(dev), coef.to(dev), feat.to(dev)


def torch_shap(bins_u8, splits, is_cat, table, f0, structure, chunk):
    own, coef, feat = structure
    F, R = bins_u8.shape
    dev = bins_u8.device
    p3 = torch.tensor(P3, device=dev, dtype=torch.float64)
    member = torch.tensor([[mask >> j & 1 for j in range(6)] for mask in range(64)], device=dev, dtype=torch.float64)
    phi = torch.zeros(F + 1, R, device=dev, dtype=torch.float64)
    for s in range(0, splits.shape[0], chunk):
        e = s + chunk
        term = (2.0 - torch_bits(bins_u8, splits[s:e], is_cat).double()) * p3[None, :, None]       # [n, 6, R]
        delta = torch.einsum("cjd,cdr->cjr", own[s:e], term)
        idx = (FULL - torch.einsum("mj,cjr->cmr", member, delta)).long()                           # [n, 64, R]
        v = table[s:e].gather(1, idx.reshape(idx.shape[0], -1)).view(idx.shape)
        phi.index_add_(0, feat[s:e].reshape(-1), torch.einsum("cjm,cmr->cjr", coef[s:e], v).reshape(-1, R))
    phi[F] = f0 + table[:splits.shape[0], FULL].sum()
    return phi


def alternate(forms, repeats, iters, warmup=2):
    runs = {name: [] for name in forms}
    for _ in range(repeats):
        for name, (fn, n) in forms.items():
            runs[name].append(events_ms(fn, warmup, n or iters)[0])
    return {name: statistics.median(v) for name, v in runs.items()}, runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=409_600)
    ap.add_argument("--weight-rows", type=int, default=600_000)
    ap.add_argument("--fit-rows", type=int, default=100_000)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--torch-chunk", type=int, default=4)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-iters", type=int, default=2)
    ap.add_argument("--out", default=os.path.join("profiles", "gbdt_explain_micro.json"))
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    num, cat, y = make_rows(a.fit_rows, 1, dev)
    clf = ObliviousBoostingClassifier(iterations=a.trees, device=dev).fit((num, cat), y)
    model, T = clf.model_, clf.tree_count_
    splits, is_cat = model.splits[:T].long(), model.is_cat.bool()
    structure = shap_structure(splits.cpu(), dev)
    players = (structure[0].sum(2) > 0).sum(1).double()
    result = {"device": torch.cuda.get_device_name(0), "rows": a.rows, "weight_rows": a.weight_rows, "columns": 12, "trees": T,
              "depth": DEPTH, "iters": a.iters, "torch_iters": a.torch_iters, "repeats": a.repeats, "torch_chunk": a.torch_chunk,
              "shap_tree_chunk": int(recsys_amd._native.lib().rsx_gbdt_shap_tree_chunk()),
              "mean_players_per_tree": float(players.mean()), "coalitions_per_row": float((2.0 ** players).sum())}
    sets = {R: clf._bins(make_rows(R, 2 + i, dev)[:2]) for i, R in enumerate(sorted({a.rows, a.weight_rows}))}
    bins = sets[a.rows]

    # the two forms agree
    w = ops.gbdt_leaf_weights(bins, model)
    assert torch.equal(w[:T], torch_leaf_weights(bins, splits, is_cat))
    plan = ops.gbdt_explain_plan(model, w)
    peak = model.leaf_values[:T].abs().amax(1).double()
    tb, pvc = torch_plan(model.leaf_values[:T], w[:T])
    assert bool(((plan.table[:T] - tb).abs().amax(1) <= 1e-14 * peak).all())
    assert bool(((plan.pvc[:T] - pvc).abs().amax(1) <= 1e-14 * w[:T].sum(1) * (2 * peak) ** 2).all())
    bound = abs(model.f0) + float(peak.sum())
    head = min(a.rows, 8192)
    few = bins[:, :head].contiguous()
    err = float((ops.gbdt_shap(few, model, plan) - torch_shap(few, splits, is_cat, plan.table, model.f0, structure,
                                                              a.torch_chunk)).abs().max())
    assert err <= 1e-12 * bound, (err, bound)
    result["shap_max_abs_difference"], result["shap_bound"] = err, 1e-12 * bound

    out = torch.empty(13, a.rows, device=dev, dtype=torch.float64)
    ms, runs = alternate({
        "shap_native": (lambda: ops.gbdt_shap(bins, model, plan, out=out), None),
        "shap_torch": (lambda: torch_shap(bins, splits, is_cat, plan.table, model.f0, structure, a.torch_chunk), a.torch_iters),
        "predict_native": (lambda: ops.gbdt_predict(bins, model), None),
        "plan_native": (lambda: ops.gbdt_explain_plan(model, w), None),
        "plan_torch": (lambda: torch_plan(model.leaf_values[:T], w[:T]), None),
    }, a.repeats, a.iters)
    for R, b in sets.items():
        m2, r2 = alternate({
            f"leaf_weights_native_{R}": (lambda: ops.gbdt_leaf_weights(b, model, out=w), None),
            f"leaf_weights_torch_{R}": (lambda: torch_leaf_weights(b, splits, is_cat), a.torch_iters),
        }, a.repeats, a.iters)
        ms.update(m2)
        runs.update(r2)
    result["ms"], result["ms_all"] = ms, runs
    result["torch_over_native"] = {"shap": ms["shap_torch"] / ms["shap_native"], "plan": ms["plan_torch"] / ms["plan_native"]}
    for R in sets:
        result["torch_over_native"][f"leaf_weights_{R}"] = ms[f"leaf_weights_torch_{R}"] / ms[f"leaf_weights_native_{R}"]
    result["shap_table_reads_per_s"] = a.rows * result["coalitions_per_row"] / (ms["shap_native"] * 1e-3)
    print(json.dumps(result, indent=1, sort_keys=True), flush=True)
    os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
