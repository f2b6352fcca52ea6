"""Integer reference of ops.binary_eval (a helper, not a test): sort the scores, walk the tie groups
and accumulate P, N and U2 in Python integers; the Logloss in float64.

U2 = sum over positive rows i of #{negative j : z_j < z_i} + #{negative j : z_j <= z_i}
(twice the Mann-Whitney U statistic with ties at one half); AUC = U2 / (2 P N)."""
import math

import numpy as np


def counts(z, y):
    """(P, N, U2) as Python ints. z: float scores (compared as reals: -0.0 == +0.0), y: 0 / 1."""
    z = np.asarray(z, dtype=np.float64).reshape(-1) + 0.0    # -0.0 + 0.0 = +0.0
    y = np.asarray(y).reshape(-1)
    assert z.shape == y.shape and np.isin(y, (0, 1)).all()
    order = np.argsort(z, kind="stable")
    zs, ys = z[order].tolist(), y[order].astype(np.int64).tolist()
    P = N = U2 = 0
    neg_before = 0
    i, R = 0, len(zs)
    while i < R:
        j, pos, neg = i, 0, 0
        while j < R and zs[j] == zs[i]:
            pos += ys[j]
            neg += 1 - ys[j]
            j += 1
        U2 += pos * (2 * neg_before + neg)
        P += pos
        N += neg
        neg_before += neg
        i = j
    return P, N, U2


def auc(z, y):
    P, N, U2 = counts(z, y)
    return U2 / (2 * P * N) if P and N else float("nan")


def logloss_sum(z, y):
    """sum_r max(z,0) - z y + log1p(exp(-|z|)) in float64 (math.fsum of the float64 rows)."""
    z = np.asarray(z, dtype=np.float64).reshape(-1)
    y = np.asarray(y, dtype=np.float64).reshape(-1)
    return math.fsum((np.maximum(z, 0.0) - z * y + np.log1p(np.exp(-np.abs(z)))).tolist())
