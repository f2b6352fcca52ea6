"""Micro-benchmark of the persona path (csrc/tx_features.hip's run / sum / ratio passes, csrc/kmeans.hip) at the
reference's scale: --rows rows (15,000,000), --customers customers (1,000,000), --items articles (70,000) generated
on the device from a seed, K = --clusters (16), d = 7.

  passes   ops.tx_segment_runs (items, categories), ops.tx_segment_sum_f64 (with and without the second pass),
           ops.tx_price_ratio, ops.standardize_columns, ops.kmeans_quantize between device events: median, minimum
           and maximum of --iters after a warm-up; the wrappers allocate their outputs, as a caller's do.
  kmeans   the seeding (K - 1 rounds), one Lloyd iteration (assignment, integer sums, new centres) and a whole fit
           (tol 1e-4, the final assignment included), each alternating with a plain-PyTorch restatement on the same
           GPU: cdist / argmin / index_add_ / bincount, and for the seeding sklearn's D^2 sampling by cumsum and
           searchsorted with one host read per round. The data are --blobs Gaussian blobs plus noise, standardised.
  frames   persona_features + cluster_personas + persona_stats by wall clock (ending in the host frames) on a host
           frame of --frame-rows rows, against the pandas / scipy / scikit-learn restatement of
           tests/persona_ref.py on this machine's CPUs.

Everything on the GPU runs inside this one process; run it under a time limit. Writes --out
(profiles/persona_micro.json)."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import pandas as pd
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import recsys_amd  # noqa: E402,F401
from recsys_amd import _native as N  # noqa: E402
from recsys_amd import ops  # noqa: E402
from recsys_amd.staticstics import preprocess_clustering as PC  # noqa: E402
from tests import persona_ref as PR  # noqa: E402
from tools.tx_features_micro import device_table, summary, timed_ms  # noqa: E402


def host_frame(rows, C, n_items, seed=1):
    rng = np.random.default_rng(seed)
    cid = np.asarray([f"{i:032x}" for i in range(C)], dtype=object)
    aid = np.asarray([f"{100 + i % 97:03d}{i:07d}" for i in range(n_items)], dtype=object)      # 97 categories
    day = np.datetime64("2019-09-23", "D") + rng.integers(0, 371, rows).astype("timedelta64[D]")
    return pd.DataFrame({"t_dat": day, "customer_id": cid[rng.integers(0, C, rows)],
                         "article_id": aid[np.minimum((n_items * rng.random(rows) ** 2.5).astype(np.int64), n_items - 1)],
                         "price": (rng.integers(1, 512, rows) / 1024.0).astype(np.float32),
                         "sales_channel_id": rng.integers(1, 3, rows).astype(np.int8)})


# ---- plain-PyTorch restatements ---------------------------------------------------------------------------------------
def torch_iteration(X, c):
    """X [C, d], c [K, d] -> (labels, new centres): one Lloyd iteration."""
    labels = torch.cdist(X, c).argmin(dim=1)
    sums = torch.zeros_like(c).index_add_(0, labels, X)
    n = torch.bincount(labels, minlength=c.shape[0]).to(X.dtype)
    return labels, torch.where(n[:, None] > 0, sums / n[:, None].clamp(min=1), c)


def torch_fit(X, c, tol_abs, max_iter=300):
    labels = torch.full((X.shape[0],), -1, device=X.device)
    for it in range(1, max_iter + 1):
        new_labels, new = torch_iteration(X, c)
        stop = bool((new_labels == labels).all()) or float(((new - c) ** 2).sum()) <= tol_abs      # the host looks, as sklearn
        labels, c = new_labels, new
        if stop:
            break
    return c, torch.cdist(X, c).argmin(dim=1), it


def torch_seed(X, K, g):
    """k-means++ by D^2 sampling through a prefix sum: one host read per round (the drawn row)."""
    rows = [int(torch.randint(0, X.shape[0], (1,), device=X.device, generator=g))]
    dmin = ((X - X[rows[0]]) ** 2).sum(dim=1)
    for _ in range(1, K):
        cum = torch.cumsum(dmin, 0)
        r = int(torch.searchsorted(cum, torch.rand(1, device=X.device, generator=g, dtype=X.dtype) * cum[-1]).clamp(max=X.shape[0] - 1))
        rows.append(r)
        dmin = torch.minimum(dmin, ((X - X[r]) ** 2).sum(dim=1))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=15_000_000)
    ap.add_argument("--customers", type=int, default=1_000_000)
    ap.add_argument("--items", type=int, default=70_000)
    ap.add_argument("--clusters", type=int, default=16)
    ap.add_argument("--blobs", type=int, default=12)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--frame-rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join("profiles", "persona_micro.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("persona_micro: no GPU")
    dev = torch.device("cuda:0")
    T, C, n_items, K, it = args.rows, args.customers, args.items, args.clusters, args.iters
    res = {"device": torch.cuda.get_device_name(0), "rows": T, "customers": C, "items": n_items, "clusters": K, "d": 7,
           "iters": it, "passes": {}, "kmeans": {}, "torch": {}}
    P = res["passes"]

    # ---- the passes --------------------------------------------------------------------------------------------------
    tab = device_table(T, C, n_items, 53, dev)
    tab.article_ids = np.asarray([f"{i // 1000:03d}{i:07d}" for i in range(n_items)])      # ascending strings, 1,000 items a category
    seg = tab.row_customer
    items_sorted = tab.items_by_customer
    item_cat = (torch.arange(n_items, device=dev) * 97 // n_items).to(torch.int32)
    cats_sorted = tab._sorted_within_customer(item_cat[tab.item.long()])
    price64 = tab.price.to(torch.float64)
    cat_mean = torch.rand(97, device=dev, dtype=torch.float64) + 0.5
    P["segment_runs_items"] = summary(timed_ms([lambda: ops.tx_segment_runs(seg, C, items_sorted)], it)[0], 32 * T + 16 * C)
    P["segment_runs_categories"] = summary(timed_ms([lambda: ops.tx_segment_runs(seg, C, cats_sorted)], it)[0], 32 * T + 16 * C)
    t_sum, t_torch = timed_ms([lambda: ops.tx_segment_sum_f64(seg, C, price64, m2=False),
                               lambda: torch.zeros(C, device=dev, dtype=torch.float64).index_add_(0, seg.long(), price64)], it)
    P["segment_sum_f64"] = summary(t_sum, 24 * T + 12 * C)
    res["torch"]["segment_sum_f64_index_add"] = summary(t_torch)
    P["segment_sum_f64_with_m2"] = summary(timed_ms([lambda: ops.tx_segment_sum_f64(seg, C, price64)], it)[0], 48 * T + 20 * C)
    t_ratio, t_torch = timed_ms([lambda: ops.tx_price_ratio(tab.item, tab.price, item_cat, cat_mean),
                                 lambda: tab.price.double() / cat_mean[item_cat[tab.item.long()].long()]], it)
    P["price_ratio"] = summary(t_ratio, 16 * T)
    res["torch"]["price_ratio"] = summary(t_torch)
    t0 = time.perf_counter()
    feats = tab.persona_features()
    torch.cuda.synchronize()
    res["persona_features_device_table_s"] = time.perf_counter() - t0      # first use: the sorts and statistics included
    tab.check()
    del tab, seg, items_sorted, cats_sorted, price64, feats
    torch.cuda.empty_cache()

    print("persona_micro: passes done", file=sys.stderr, flush=True)

    # ---- k-means -------------------------------------------------------------------------------------------------------
    g = torch.Generator(device=dev).manual_seed(3)
    centres = 6.0 * torch.randn(args.blobs, 7, device=dev, generator=g, dtype=torch.float64)
    X = centres[torch.randint(0, args.blobs, (C,), device=dev, generator=g)] + torch.randn(C, 7, device=dev, generator=g, dtype=torch.float64)
    Xt = X.t().contiguous()
    P["standardize_columns"] = summary(timed_ms([lambda: ops.standardize_columns(Xt)], it)[0], 4 * 56 * C)
    Z = ops.standardize_columns(Xt)[0]
    P["kmeans_quantize"] = summary(timed_ms([lambda: ops.kmeans_quantize(Z)], it)[0], 2 * 56 * C + 28 * C)
    q, bits = ops.kmeans_quantize(Z)
    grid_x = (q.to(torch.float64) * 2.0 ** -bits).t().contiguous()          # [C, d]: what both sides cluster
    tol_abs = 1e-4 * float(ops.standardize_columns(grid_x.t().contiguous(), out=False)[3].mean())
    t_seed, t_torch = timed_ms([lambda: ops.kmeans_seed(q, bits, K, 42), lambda: torch_seed(grid_x, K, g)], it)
    res["kmeans"]["seed"] = summary(t_seed)
    res["torch"]["seed_cumsum_searchsorted"] = summary(t_torch)
    init = ops.kmeans_seed(q, bits, K, 42)[1]

    labels = torch.full((C,), -1, device=dev, dtype=torch.int32)
    sum_q = torch.zeros(K, 7, device=dev, dtype=torch.int64)
    count = torch.zeros(K, device=dev, dtype=torch.int32)
    ctl = torch.zeros(4, device=dev, dtype=torch.int32)
    shift = torch.zeros(1, device=dev, dtype=torch.float64)
    work = init.clone()
    groups = 4 * ops.num_cus(dev)

    def one_iteration():
        work.copy_(init)
        ctl.zero_()
        N.check(N.lib().rsx_kmeans_iterate(N.ptr(q), 7, C, bits, K, N.ptr(work), N.ptr(labels), N.ptr(sum_q), N.ptr(count),
                                           N.ptr(ctl), N.ptr(shift), 0.0, 1, 1, groups, N.stream()), "kmeans_iterate")

    t_it, t_torch = timed_ms([one_iteration, lambda: torch_iteration(grid_x, init)], it)
    res["kmeans"]["one_iteration"] = summary(t_it, 28 * C + 8 * C)
    res["torch"]["one_iteration"] = summary(t_torch)
    t_as, t_torch = timed_ms([lambda: ops.kmeans_assign(q, bits, init), lambda: torch.cdist(grid_x, init).min(dim=1)], it)
    res["kmeans"]["assign_with_inertia"] = summary(t_as, 28 * C + 12 * C)
    res["torch"]["assign_cdist_min"] = summary(t_torch)
    fit = ops.kmeans_fit(q, bits, init, tol_abs)
    c_t, l_t, n_t = torch_fit(grid_x, init, tol_abs)
    res["kmeans"]["fit_iterations"], res["torch"]["fit_iterations"] = fit.n_iter, n_t
    res["fit_labels_equal_torch"] = float((fit.labels.long() == l_t).double().mean())
    n_fit = max(3, it // 4)
    t_fit, t_torch = timed_ms([lambda: ops.kmeans_fit(q, bits, init, tol_abs), lambda: torch_fit(grid_x, init, tol_abs)], n_fit, warm=1)
    res["kmeans"]["fit"] = summary(t_fit)
    res["torch"]["fit"] = summary(t_torch)
    del X, Xt, Z, q, grid_x, labels
    torch.cuda.empty_cache()

    print("persona_micro: k-means done", file=sys.stderr, flush=True)

    # ---- end to end on a host frame --------------------------------------------------------------------------------------
    scale = args.frame_rows / T
    df = host_frame(args.frame_rows, max(int(C * scale), 1000), max(int(n_items * min(1.0, 4 * scale)), 500))

    def build():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        table = PC.TransactionTable.from_frame(df, dev)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        feats = PC.persona_features(table)
        t2 = time.perf_counter()
        labels, _, _, _ = PC.cluster_personas(feats, n_clusters=K, random_state=42)
        t3 = time.perf_counter()
        PC.persona_stats(feats, labels)
        t4 = time.perf_counter()
        return {"from_frame_s": t1 - t0, "persona_features_s": t2 - t1, "cluster_personas_s": t3 - t2, "persona_stats_s": t4 - t3,
                "total_s": t4 - t0}

    build()                                                                    # warm-up
    runs = [build() for _ in range(3)]
    res["frames"] = {"rows": args.frame_rows, "customers": int(df["customer_id"].nunique()), "items": int(df["article_id"].nunique()),
                     "runs": runs, "median_total_s": statistics.median(r["total_s"] for r in runs)}
    print("persona_micro: device frames done", file=sys.stderr, flush=True)
    from sklearn.cluster import KMeans
    from sklearn.preprocessing import StandardScaler
    t0 = time.perf_counter()
    feats = PR.features(df)
    t1 = time.perf_counter()
    Zs = StandardScaler().fit_transform(feats[PR.COLS])
    km_labels = KMeans(n_clusters=K, random_state=42).fit_predict(Zs)
    t2 = time.perf_counter()
    PR.persona_json(feats, km_labels)
    t3 = time.perf_counter()
    res["host_restatement"] = {"rows": args.frame_rows, "cpus_available": int(os.environ.get("OMP_NUM_THREADS") or os.cpu_count() or 1),
                               "features_s": t1 - t0, "scaler_and_kmeans_s": t2 - t1, "persona_json_s": t3 - t2, "total_s": t3 - t0}
    res["host_over_device"] = res["host_restatement"]["total_s"] / res["frames"]["median_total_s"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
