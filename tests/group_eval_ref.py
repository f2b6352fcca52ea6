"""Per-group reference of ops.group_eval (a helper, not a test): sort the rows by (group, -score),
walk every group's tie groups and accumulate P, N and U2 in Python integers, the tie-averaged DCG@top
by math.fsum over the tie groups' terms (the table D of ops.ndcg_discounts, shared with the device),
and the two means by math.fsum.

With the group sorted by descending score, a tie group at the 0-based positions [s, e] holding pos
positives and neg negatives, and nb negatives above it:
  V2 += pos * (2 nb + neg)   (negatives scored higher, twice, + the tied ones once)
  DCG += pos * (D[min(e + 1, top)] - D[min(s, top)]) / (e - s + 1)
U2 = 2 P N - V2 (twice the tie-aware Mann-Whitney U); AUC_g = U2 / (2 P N); NDCG_g = DCG / D[min(P, top)]."""
import math

import numpy as np

from recsys_amd import ops


def per_group(z, y, g, top):
    """[{"gid", "rows", "P", "N", "U2", "dcg"}] ascending by group id."""
    z = np.asarray(z, dtype=np.float64).reshape(-1) + 0.0    # -0.0 + 0.0 = +0.0
    y = np.asarray(y).reshape(-1)
    g = np.asarray(g).reshape(-1).astype(np.int64)
    assert z.shape == y.shape == g.shape and np.isin(y, (0, 1)).all()
    D = ops.ndcg_discounts(top).tolist()
    order = np.lexsort((-z, g))
    zs, ys, gs = z[order].tolist(), y[order].astype(np.int64).tolist(), g[order].tolist()
    out, i, R = [], 0, len(zs)
    while i < R:
        j = i
        while j < R and gs[j] == gs[i]:
            j += 1
        P = N = V2 = 0
        terms = []
        s = i
        while s < j:
            e, pos = s, 0
            while e < j and zs[e] == zs[s]:
                pos += ys[e]
                e += 1
            neg = (e - s) - pos
            V2 += pos * (2 * N + neg)
            if pos:
                terms.append(pos * (D[min(e - i, top)] - D[min(s - i, top)]) / (e - s))
            P += pos
            N += neg
            s = e
        out.append({"gid": gs[i], "rows": j - i, "P": P, "N": N, "U2": 2 * P * N - V2, "dcg": math.fsum(terms)})
        i = j
    return out


def summary(groups, top):
    """{"ndcg", "query_auc", "groups", "ndcg_groups", "auc_groups"} of per_group's list."""
    D = ops.ndcg_discounts(top).tolist()
    nd = [r["dcg"] / D[min(r["P"], top)] for r in groups if r["P"] > 0]
    au = [r["U2"] / (2 * r["P"] * r["N"]) for r in groups if r["P"] > 0 and r["N"] > 0]
    return {"ndcg": math.fsum(nd) / len(nd) if nd else float("nan"),
            "query_auc": math.fsum(au) / len(au) if au else float("nan"),
            "groups": len(groups), "ndcg_groups": len(nd), "auc_groups": len(au)}
