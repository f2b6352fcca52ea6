"""Customer personas from the transaction log (reference staticstics/preprocess_clustering.py): seven behaviour
columns per customer, standardised, clustered by k-means, and each cluster described by its statistics and a tag
name: the persona JSON (cluster_id, persona_name, stats, user_count) the product side reads.

The reference is a script over module-level dummy data: pandas groupby().apply(value_counts) per customer, then
scikit-learn's StandardScaler and KMeans on the host. Here it is functions. The columns come from a TransactionTable
(TransactionTable.persona_features: segmented scans of csrc/tx_features.hip, no loop over customers), the clustering
is csrc/kmeans.hip: k-means on a fixed-point grid whose cluster sums are integers, so a fit gives the same bits
every run and in any row order (include/recsys_amd.h, "k-means"; tests/persona_ref.py restates it in numpy).

Definitions where the reference leaves a choice ("personas"): the head items of long_tail_ratio break
count ties by ascending item index; prices are the log's float32 values; the seeds are drawn by k-means++ from the
library's counter-based hash, not from scikit-learn's random stream, so cluster numbers differ from the
reference's while the method does not; an empty cluster keeps its centre (scikit-learn relocates it)."""
from __future__ import annotations

import json

import numpy as np
import pandas as pd
import torch

from .. import ops
from .preprosess_agg_parallel import TransactionTable, _ids, _table

COLS_FOR_CLUSTER = list(ops.PERSONA_COLUMNS)


def persona_features(train_df, device=None) -> pd.DataFrame:
    """customer_id and the seven columns COLS_FOR_CLUSTER (float64), one row per customer of the log in ascending
    customer_id order; train_df is the transactions frame or a prepared TransactionTable."""
    tab = _table(train_df, device)
    cols = tab.persona_features().cpu().numpy()
    tab.check()
    out = pd.DataFrame({"customer_id": _ids(tab.customer_ids)})
    for k, name in enumerate(COLS_FOR_CLUSTER):
        out[name] = cols[k]
    return out


def _feature_major(X, device=None) -> torch.Tensor:
    """X [C, d], a host array or a device tensor -> fp64 [d, C] on the device, contiguous (the one transpose)."""
    if torch.is_tensor(X):
        t = X if device is None else X.to(device)
    else:
        t = torch.from_numpy(np.ascontiguousarray(np.asarray(X, dtype=np.float64)))
        t = t.to(torch.device("cuda" if device is None else device))
    if t.dim() != 2 or t.numel() == 0:
        raise ValueError(f"expected a non-empty [n_samples, n_features] matrix, got shape {tuple(t.shape)}")
    return t.to(torch.float64).t().contiguous()


class DeviceKMeans:
    """sklearn.cluster.KMeans' surface (fit, fit_predict, predict, cluster_centers_, labels_, inertia_, n_iter_) on
    ops.kmeans_*: Lloyd's algorithm from k-means++ seeds on the grid 2^-frac_bits_ (the data are rounded to it once;
    frac_bits_ = min(20, 30 - ceil(log2 max|x|)), at least 2^-20 apart for standardised columns). tol is sklearn's:
    the fit stops when the centres' squared shift is <= tol * the mean column variance, or when no label changes.
    Run r of n_init uses the seed random_state + 1000 r; the smallest inertia wins, the lowest run on ties. init: an
    optional [n_clusters, d] array of starting centres (then n_init is 1). X is [n_samples, n_features], a host
    array or a device tensor."""

    def __init__(self, n_clusters=8, random_state=42, n_init=1, max_iter=300, tol=1e-4, init=None, device=None):
        if int(n_clusters) < 1 or int(n_init) < 1 or int(max_iter) < 1 or not float(tol) >= 0.0:
            raise ValueError("DeviceKMeans: need n_clusters >= 1, n_init >= 1, max_iter >= 1 and tol >= 0")
        self.n_clusters, self.random_state, self.n_init = int(n_clusters), int(random_state), int(n_init)
        self.max_iter, self.tol, self.init, self.device = int(max_iter), float(tol), init, device

    def fit_feature_major(self, Xt):
        """fit on fp64 [d, C] device data (no transpose)."""
        d, C = Xt.shape
        if C < self.n_clusters:
            raise ValueError(f"DeviceKMeans: n_samples={C} should be >= n_clusters={self.n_clusters}")
        q, bits = ops.kmeans_quantize(Xt)
        grid = q.to(torch.float64) * 2.0 ** -bits
        tol_abs = self.tol * float(ops.standardize_columns(grid, out=False)[3].mean())
        best = None
        if self.init is not None:
            starts = [torch.as_tensor(np.asarray(self.init, dtype=np.float64)).to(Xt.device).contiguous()]
            if tuple(starts[0].shape) != (self.n_clusters, d):
                raise ValueError(f"DeviceKMeans: init must be [{self.n_clusters}, {d}], got {tuple(starts[0].shape)}")
        else:
            starts = [None] * self.n_init
        for r, start in enumerate(starts):
            if start is None:
                start = ops.kmeans_seed(q, bits, self.n_clusters, self.random_state + 1000 * r)[1]
            fit = ops.kmeans_fit(q, bits, start, tol_abs, self.max_iter)
            inertia = float(fit.inertia)
            if best is None or inertia < best[0]:
                best = (inertia, fit)
        self.inertia_, fit = best
        self.frac_bits_, self.n_iter_, self.n_features_in_ = bits, fit.n_iter, d
        self.centres_device, self.labels_device = fit.centres, fit.labels
        self.cluster_centers_ = fit.centres.cpu().numpy()
        self.labels_ = fit.labels.cpu().numpy()
        return self

    def fit(self, X, y=None):
        return self.fit_feature_major(_feature_major(X, self.device))

    def fit_predict(self, X, y=None):
        return self.fit(X).labels_

    def predict(self, X):
        """The nearest centre of every row, on the fit's grid (a value that does not fit it raises ValueError)."""
        if not hasattr(self, "centres_device"):
            raise RuntimeError("DeviceKMeans: predict before fit")
        Xt = _feature_major(X, self.centres_device.device)
        if Xt.shape[0] != self.n_features_in_:
            raise ValueError(f"DeviceKMeans: X has {Xt.shape[0]} features, the fit had {self.n_features_in_}")
        q, _ = ops.kmeans_quantize(Xt, self.frac_bits_)
        return ops.kmeans_assign(q, self.frac_bits_, self.centres_device, inertia=False)[0].cpu().numpy()


def cluster_personas(features, n_clusters=10, random_state=42, device=None):
    """StandardScaler then KMeans over COLS_FOR_CLUSTER of the features frame (:121-134): (labels int32 [C], the
    fitted DeviceKMeans, scaler mean [7], scaler scale [7])."""
    X = _feature_major(features[COLS_FOR_CLUSTER].to_numpy(dtype=np.float64), device)
    Z, mean, scale, _ = ops.standardize_columns(X)
    model = DeviceKMeans(n_clusters=n_clusters, random_state=random_state, device=device).fit_feature_major(Z)
    return model.labels_, model, mean.cpu().numpy(), scale.cpu().numpy()


def _r2(x) -> float:
    """The reference's round(value, 2) of a numpy float64 (numpy's rounding, not Python's)."""
    return float(round(np.float64(x), 2))


def describe_personas(means, basket_std, counts, global_means) -> list:
    """The persona list (:141-202) from the per-cluster means [K, 7] in the order COLS_FOR_CLUSTER, basket_size's
    standard deviation [K] (NaN for a cluster of one: 0.0), the user counts [K] and the global means [7]. Host only.
    A cluster without users is left out."""
    means, basket_std = np.asarray(means, dtype=np.float64), np.asarray(basket_std, dtype=np.float64)
    global_avg_price = float(np.asarray(global_means, dtype=np.float64)[COLS_FOR_CLUSTER.index("avg_price")])
    out = []
    for k in range(len(means)):
        if int(counts[k]) == 0:
            continue
        stats = {name: _r2(means[k, j]) for j, name in enumerate(COLS_FOR_CLUSTER)}
        std = _r2(basket_std[k])
        if np.isnan(std):
            std = 0.0
        desc = []
        if stats["weekend_ratio"] > 0.6:
            desc.append("Weekend_Shopper")
        elif stats["weekend_ratio"] < 0.3:
            desc.append("Weekday_Shopper")
        if stats["repurchase_rate"] > 0.3:
            desc.append("Loyal_Rebuyer")
        if stats["relative_price_pos"] < 0.9:
            desc.append("Discount_Hunter")
        elif stats["relative_price_pos"] > 1.1:
            desc.append("Premium_Picker")
        if stats["cat_entropy"] < 0.5:
            desc.append("Specialist")
        elif stats["cat_entropy"] > 1.5:
            desc.append("Explorer")
        if stats["long_tail_ratio"] > 0.6:
            desc.append("Hipster")
        if not desc:
            desc.append("Standard_Shopper")
        out.append({
            "cluster_id": int(k),
            "persona_name": f"Cluster {k}: {' & '.join(desc)}",
            "stats": {
                "basket_size": {"mean": stats["basket_size"], "std": std},
                "category_entropy": stats["cat_entropy"],
                "price_sensitivity": {
                    "avg_price": stats["avg_price"],
                    "relative_pos": stats["relative_price_pos"],
                    "description": "High Spending" if stats["avg_price"] > global_avg_price else "Low Spending",
                },
                "shopping_pattern": {
                    "weekend_ratio": stats["weekend_ratio"],
                    "repurchase_rate": stats["repurchase_rate"],
                    "long_tail_ratio": stats["long_tail_ratio"],
                },
            },
            "user_count": int(counts[k]),
        })
    return out


def persona_stats(features, labels, n_clusters=None, device=None) -> list:
    """The persona list of a clustering: per cluster the means of the seven columns, basket_size's standard
    deviation (ddof = 1) and the user count, by one stable device sort of the labels and ops.tx_segment_sum_f64 per
    column; the global means by the fixed-order column sums. One host read (the K x 9 statistics and the global
    means), then describe_personas."""
    X = _feature_major(features[COLS_FOR_CLUSTER].to_numpy(dtype=np.float64), device)
    lab = torch.as_tensor(np.asarray(labels.cpu()) if torch.is_tensor(labels) else np.asarray(labels)).to(torch.int32).to(X.device)
    if lab.dim() != 1 or lab.numel() != X.shape[1]:
        raise ValueError(f"persona_stats: {lab.numel()} labels for {X.shape[1]} customers")
    K = int(lab.max()) + 1 if n_clusters is None else int(n_clusters)
    order = torch.sort(lab, stable=True)
    seg, perm = order.values.contiguous(), order.indices.contiguous()
    rows = []
    for j in range(len(COLS_FOR_CLUSTER)):
        count, total, m2 = ops.tx_segment_sum_f64(seg, K, X[j], perm=perm, m2=j == 0)
        n = count.to(torch.float64)
        rows.append(total / n)
        if j == 0:
            std = torch.sqrt(m2 / (n - 1.0))          # NaN for a cluster of one, as pandas' std
    ops._TX_SUM_GUARD.check()
    table = torch.stack(rows + [std, n], dim=1)                       # [K, 9]
    global_means = ops.standardize_columns(X, out=False)[1]
    host = torch.cat([table, torch.cat([global_means, global_means.new_zeros(2)])[None]]).cpu().numpy()
    stats, g = host[:K], host[K, :len(COLS_FOR_CLUSTER)]
    return describe_personas(stats[:, :7], stats[:, 7], stats[:, 8].astype(np.int64), g)


def personas_json(stats, save_path=None) -> str:
    """The reference's json.dumps(stats, indent=2, ensure_ascii=False); written to save_path when given."""
    text = json.dumps(stats, indent=2, ensure_ascii=False)
    if save_path is not None:
        with open(save_path, "w", encoding="utf-8") as f:
            f.write(text)
    return text


__all__ = ["COLS_FOR_CLUSTER", "TransactionTable", "persona_features", "DeviceKMeans", "cluster_personas",
           "describe_personas", "persona_stats", "personas_json"]
