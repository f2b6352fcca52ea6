"""Micro-benchmark of the ranker's training rows (csrc/ranker_rows.hip) at HMLogImporter's default size:
--positives purchases x (1 + --neg) rows (100,000 x 6 = 600,000, tools/gbdt_micro.py's row count), --items
items and --customers customers of d = 128.

  kernels  rsx_ranker_rows_sample and rsx_pair_tabular called on preallocated outputs between device events
           (median of --iters after a warm-up), their rows/s, and the bytes each row needs by the model below
           over that time as a fraction of the HBM peak (8.0 TB/s) and of the measured copy rate (6.29 TB/s):
             sample  12 B written (user, item, y) + 8 B per positive read = 12 + 8 / (1 + neg) B per row
                     (the offsets and the bought list, one binary search per negative, are shared by a
                     customer's rows and counted as cached);
             pair    8 B of ids + 2 x 4 d B of vectors + 8 B of price and average + 28 B written = 44 + 8 d B
                     per row. The vectors are counted as requested: a customer's rows follow one another and
                     the item table may sit in the Infinity Cache, so this is a rate of requested bytes, not
                     of HBM traffic.
  serving  rsx_pair_tabular against rsx_rerank_tabular on the same pairs (one query per positive, 1 + neg
           candidates, the score given), the two alternating; both medians and each one's spread.
  logs -> model  a CSV of --positives lines -> HMLogImporter.load_rows -> RecommendationRanker.train_rows
           (--trees trees), host clock ending in a synchronise, against the path that existed before: the same
           rows as FeatureEngineer dicts -> RecommendationRanker.train (prepare_batch, a pandas frame, fit),
           at --host-positives purchases (default: the same count).

Writes --out (profiles/ranker_rows_micro.json)."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import recsys_amd  # noqa: E402,F401
from recsys_amd import _native as N  # noqa: E402
from recsys_amd import ops  # noqa: E402
from recsys_amd.temp_model.ranker_skelet import RecommendationRanker  # noqa: E402
from recsys_amd.utils.monitor.log_importer import HMLogImporter  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12
CATEGORY, MATERIAL, FIT = tuple(f"cat{i}" for i in range(40)), tuple(f"mat{i}" for i in range(12)), ("slim", "regular", "loose")
SEASON, GENDER = ("SS", "FW", "AW", "HS"), ("F", "M", "U")


def timed_ms(fns, iters, warm=3):
    """Device-event times (ms) of the callables, run alternately: a list of `iters` times per callable."""
    for _ in range(warm):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    out = [[] for _ in fns]
    for _ in range(iters):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            out[k].append(e0.elapsed_time(e1))
    return out


def summary(ms, rows, bytes_per_row):
    med = statistics.median(ms)
    return {"median_ms": med, "min_ms": min(ms), "max_ms": max(ms), "spread": (max(ms) - min(ms)) / med,
            "rows_per_s": rows / (med * 1e-3), "bytes_per_row": bytes_per_row,
            "requested_bytes_per_s": rows * bytes_per_row / (med * 1e-3),
            "fraction_of_hbm_peak": rows * bytes_per_row / (med * 1e-3) / HBM_PEAK,
            "fraction_of_measured_copy_rate": rows * bytes_per_row / (med * 1e-3) / HBM_COPY}


def make_log(args, rng):
    """[(customer, item)] of --positives purchases: customers uniform, items Zipf-like."""
    cust = rng.integers(0, args.customers, args.positives)
    item = np.minimum((rng.pareto(1.2, args.positives) * args.items / 50).astype(np.int64), args.items - 1)
    return cust, rng.permutation(args.items)[item]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--positives", type=int, default=100000)
    ap.add_argument("--host-positives", type=int, default=None)
    ap.add_argument("--neg", type=int, default=5)
    ap.add_argument("--items", type=int, default=105542)
    ap.add_argument("--customers", type=int, default=20000)
    ap.add_argument("--trees", type=int, default=1000)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join("profiles", "ranker_rows_micro.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("ranker_rows_micro: no GPU")
    dev = torch.device("cuda:0")
    d, K = 128, args.neg
    rng = np.random.default_rng(0)
    V = rng.standard_normal((args.items, d)).astype(np.float32)
    V /= np.linalg.norm(V, axis=1, keepdims=True)
    U = rng.standard_normal((args.customers, d)).astype(np.float32)
    U /= np.linalg.norm(U, axis=1, keepdims=True)
    items = {i: {"category": CATEGORY[c], "material": MATERIAL[m], "fit": FIT[f], "price": float(p) / 4}
             for i, (c, m, f, p) in enumerate(zip(rng.integers(0, 40, args.items), rng.integers(0, 12, args.items),
                                                  rng.integers(0, 3, args.items), rng.integers(4, 400, args.items)))}
    users = [{"season": SEASON[s], "gender": GENDER[g], "avg_price": float(2 ** a)}
             for s, g, a in zip(rng.integers(0, 4, args.customers), rng.integers(0, 3, args.customers),
                                rng.integers(3, 7, args.customers))]
    keys = [f"{100000000 + 7 * i:010d}" for i in range(args.items)]
    customers = [f"{i:064x}" for i in range(args.customers)]
    cust, item = make_log(args, rng)
    tmp = tempfile.mkdtemp()
    csv = os.path.join(tmp, "transactions.csv")
    with open(csv, "w") as f:
        f.write("t_dat,customer_id,article_id,price,sales_channel_id\n")
        f.writelines(f"2020-09-01,{customers[c]},{keys[i]},0.05,2\n" for c, i in zip(cust.tolist(), item.tolist()))
    store = dict(zip(keys, V))
    dU, dV = torch.from_numpy(U).to(dev), torch.from_numpy(V).to(dev)
    index = {c: i for i, c in enumerate(customers)}
    imp = HMLogImporter(csv, store, device=dev)
    res = {"device": torch.cuda.get_device_name(0), "positives": args.positives, "negative_ratio": K, "items": args.items,
           "customers": args.customers, "d": d, "iters": args.iters, "trees": args.trees}

    # ---- the two kernels, and the serving kernel on the same pairs ------------------------------------
    log = imp.read_log(args.positives)
    up = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
    pos_c, pos_i, off, bought = up(log["pos_customer"]), up(log["pos_item"]), up(log["bought_off"]), up(log["bought"])
    Pv, C = pos_c.numel(), off.numel() - 1
    R = Pv * (K + 1)
    res.update(rows=R, log_customers=C, longest_bought_list=int(np.diff(log["bought_off"]).max()))
    row_user = torch.empty(R, device=dev, dtype=torch.int32)
    row_item, y = torch.empty_like(row_user), torch.empty(R, device=dev)
    flag = torch.zeros(1, device=dev, dtype=torch.int32)
    lib, st = N.lib(), N.stream()

    def sample():
        N.check(lib.rsx_ranker_rows_sample(N.ptr(pos_c), N.ptr(pos_i), Pv, N.ptr(off), N.ptr(bought), bought.numel(), C,
                                           args.items, K, 42, N.ptr(row_user), N.ptr(row_item), N.ptr(y), N.ptr(flag), st))

    sample()
    want = ops.ranker_sample_rows(pos_c, pos_i, off, bought, args.items, K, 42)
    assert torch.equal(want[0], row_user) and torch.equal(want[1], row_item) and torch.equal(want[2], y)
    assert int(flag.item()) == 0
    res["sample"] = summary(timed_ms([sample], args.iters)[0], R, 12 + 8 / (K + 1))

    user_of_log = up(np.asarray([index[c] for c in log["customer_ids"]], np.int32))
    pair_user = user_of_log.index_select(0, row_user.long())           # rows of U
    price = torch.tensor([items[i]["price"] for i in range(args.items)], device=dev)
    avg = torch.tensor([m["avg_price"] for m in users], device=dev)
    score = torch.randn(R, device=dev)
    feats, serve = torch.empty(7, R, device=dev), torch.empty(7, R, device=dev)
    ids = torch.empty(R, device=dev, dtype=torch.int64)
    cand = row_item.long().view(Pv, K + 1).contiguous()
    q_user = pair_user.view(Pv, K + 1)[:, 0].long()
    Uq, avg_q = dU.index_select(0, q_user).contiguous(), avg.index_select(0, q_user).contiguous()

    def pair(sc=score):
        N.check(lib.rsx_pair_tabular(N.ptr(pair_user), N.ptr(row_item), N.ptr(sc), N.ptr(dU), N.ptr(dV), N.ptr(price),
                                     N.ptr(avg), R, args.customers, args.items, d, None, None, 0, N.ptr(feats), None,
                                     N.ptr(flag), st))

    def rerank():
        N.check(lib.rsx_rerank_tabular(N.ptr(cand), N.ptr(score), N.ptr(Uq), N.ptr(dV), N.ptr(price), N.ptr(avg_q), Pv, K + 1,
                                       args.items, d, N.ptr(serve), N.ptr(ids), N.ptr(flag), st))

    pair()
    rerank()
    assert torch.equal(feats, serve) and int(flag.item()) == 0          # the same bits on the same pairs
    t_pair, t_rerank = timed_ms([pair, rerank], args.iters)
    res["pair_tabular"] = summary(t_pair, R, 44 + 8 * d)
    res["rerank_tabular"] = summary(t_rerank, R, 44 + 8 * d)
    res["pair_over_rerank_rows_per_s"] = res["pair_tabular"]["rows_per_s"] / res["rerank_tabular"]["rows_per_s"]
    res["pair_tabular_dot_score"] = summary(timed_ms([lambda: pair(None)], args.iters)[0], R, 40 + 8 * d)

    # ---- logs -> fitted model --------------------------------------------------------------------------
    def device_path():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rows = imp.load_rows(limit=args.positives, negative_ratio=K, seed=42, user_vectors=dU, customer_index=index)
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ranker = RecommendationRanker(backend="native")
        ranker.model.iterations = args.trees
        ranker.train_rows(rows, dV, dU, items, users)
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        return rows, ranker, {"load_rows_s": t1 - t0, "train_rows_s": t2 - t1, "total_s": t2 - t0}

    device_path()                                                       # warm-up: code objects, pandas
    rows, ranker, res["device_path"] = device_path()
    ops._RANKER_ROWS_GUARD.check()
    ops._PAIR_GUARD.check()

    hp = args.positives if args.host_positives is None else args.host_positives
    n = hp * (K + 1)
    ru, ri, yy = rows.row_user[:n].cpu().numpy(), rows.row_item[:n].cpu().numpy(), rows.y[:n].cpu().numpy()
    t0 = time.perf_counter()
    dots = np.einsum("rd,rd->r", U[ru], V[ri])
    dicts = [{"user_meta": users[u], "item_meta": items[i], "two_tower_score": float(s), "user_vector": U[u],
              "item_vector": V[i], "label": int(l)} for u, i, s, l in zip(ru.tolist(), ri.tolist(), dots.tolist(), yy.tolist())]
    t1 = time.perf_counter()
    host = RecommendationRanker(backend="native")
    host.model.iterations = args.trees
    t2 = time.perf_counter()
    host.train(dicts)
    torch.cuda.synchronize()
    t3 = time.perf_counter()
    res["host_path"] = {"rows": n, "dict_build_s": t1 - t0, "train_s": t3 - t2}
    if n == len(rows):
        res["host_train_over_device_total"] = res["host_path"]["train_s"] / res["device_path"]["total_s"]
    else:
        res["host_path"]["note"] = f"the host path ran on the first {n} of {len(rows)} rows"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res, sort_keys=True))


if __name__ == "__main__":
    main()
