"""Oblivious-tree gradient boosting on the device: the classifier behind the reference's rerank stage.

Reference: RecommendationRanker (temp_model/ranker_skelet.py:95-149) boosts 1000 symmetric trees of depth 6
with CatBoostClassifier (learning_rate 0.05, Logloss, eval_metric AUC, early_stopping_rounds 50,
use_best_model) over the FeatureEngineer columns. CatBoost's GPU trainer is CUDA-only, so on an MI355X
`ObliviousBoostingClassifier` takes its place behind the same calls (fit with eval_set, predict_proba,
save_model / load_model, best_iteration_, evals_result_). It is a model of its own, specified in
include/recsys_amd.h ("oblivious-tree boosting") and restated by tests/gbdt_ref.py: plain (not ordered)
boosting, quantile-free borders at the midpoints of the distinct values, categorical columns as one-hot
candidates over host-built codes, no feature combinations. With one_hot_max_size (CatBoost's name) a
categorical column with more known values than that is encoded by ordered target statistics instead
(include/recsys_amd.h, "ordered target statistics"; ops.gbdt_ts_plan, ops.gbdt_ordered_ts; restated by
tests/gbdt_ts_ref.py): one permutation and one prior, and the column is numeric from there on. Parity with
CatBoost's own trees is not claimed.

Compute: ops.gbdt_bin (borders -> bins), ops.gbdt_tree (one native call per tree: rsx_gbdt_grad,
rsx_gbdt_histogram, rsx_gbdt_best_split, rsx_gbdt_apply_split), ops.gbdt_predict; the metrics on
ops.binary_eval / ops.group_eval. Every sum is an integer sum, so two fits of the same data give the same
model bit for bit.

`ObliviousBoostingRanker` is the same model trained on the listwise QuerySoftMax objective over the
reference's per-customer groups (utils/monitor/log_importer.py: X_user, X_item, y, groups): ops.GBDTGroupPlan,
ops.gbdt_tree(groups=...) (rsx_gbdt_tree_grouped: rsx_gbdt_grad_query_softmax in place of rsx_gbdt_grad),
ops.query_softmax_eval; restated by tests/gbdt_rank_ref.py. The two classes share everything but fit.

Explanations (include/recsys_amd.h, "explaining the boosted ranker"; csrc/gbdt_explain.hip; restated by
tests/gbdt_explain_ref.py): a fit ends by counting the training rows per leaf (leaf_weights_, CatBoost's leaf
weights; ops.gbdt_leaf_weights), and get_feature_importance gives CatBoost's "PredictionValuesChange" (also
feature_importances_), exact path-dependent "ShapValues" (ops.gbdt_explain_plan, ops.gbdt_shap) and the
SHAP-based "LossFunctionChange", in feature_names_ order. A model loaded from a file written before the
weights existed needs calc_leaf_weights(X) first.
"""
from __future__ import annotations

import math

import numpy as np
import torch

from .. import ops
from .ranker_skelet import _fit_args, _fit_eval_groups, _fit_eval_labels, _parse_eval_metric

_MAX_CODES = 255     # known values of a categorical column: codes 1..255, 0 = unknown / unseen


def build_borders(x, border_count=ops.GBDT_MAX_BORDERS):
    """The borders of the numeric columns x [Fn, R] (fp32, any device; no host read): (borders fp32
    [Fn, 256] ascending and padded with +inf, n_borders int32 [Fn]). A column's borders are the midpoints
    a/2 + b/2 of its consecutive distinct non-NaN values; with more than border_count midpoints, those at
    the ranks ((2 j + 1) (m - 1)) // (2 border_count), j < border_count, of the m - 1."""
    if not 1 <= border_count <= ops.GBDT_MAX_BORDERS:
        raise ValueError(f"border_count must be in [1, {ops.GBDT_MAX_BORDERS}] (got {border_count})")
    Fn, R = x.shape
    dev = x.device
    xs, _ = torch.sort(x, dim=1)                      # NaN sorts last
    first = ~torch.isnan(xs)
    first[:, 1:] &= xs[:, 1:] != xs[:, :-1]           # the first occurrence of every distinct value
    rank = torch.cumsum(first, 1) - 1
    distinct = torch.full((Fn, R + 1), float("inf"), device=dev, dtype=torch.float32)
    distinct.scatter_(1, torch.where(first, rank, torch.full_like(rank, R)), xs)   # slot R takes the repeats
    mids = (first.sum(1) - 1).clamp(min=0)            # midpoints a column has
    n_borders = mids.clamp(max=border_count)
    j = torch.arange(border_count, device=dev, dtype=torch.int64)[None, :]
    idx = torch.where(mids[:, None] <= border_count, j, ((2 * j + 1) * mids[:, None]) // (2 * border_count))
    idx = idx.clamp(min=0, max=R - 1)
    mid = distinct.gather(1, idx) * 0.5 + distinct.gather(1, idx + 1) * 0.5
    borders = torch.full((Fn, ops.GBDT_BINS), float("inf"), device=dev, dtype=torch.float32)
    borders[:, :border_count] = torch.where(j < n_borders[:, None], mid, torch.full_like(mid, float("inf")))
    return borders, n_borders.to(torch.int32)


def _is_frame(X):
    return hasattr(X, "columns") and hasattr(X, "iloc")


class _ObliviousBoosting:
    """What the classifier and the ranker share: the hyper-parameters, columns -> borders, vocabularies and
    bins, the raw scores and the model file. A subclass names its loss_function and brings fit."""

    loss_function = None

    def __init__(self, iterations=1000, learning_rate=0.05, depth=6, l2_leaf_reg=3.0, border_count=254,
                 cat_features=None, early_stopping_rounds=None, metric_period=1, device=None, one_hot_max_size=None,
                 ts_prior=(0.5, 1.0), ts_seed=0):
        if iterations < 1:
            raise ValueError("iterations must be >= 1")
        if not 1 <= depth <= ops.GBDT_MAX_DEPTH:
            raise ValueError(f"depth must be in [1, {ops.GBDT_MAX_DEPTH}] (got {depth})")
        if not l2_leaf_reg > 0:
            raise ValueError("l2_leaf_reg must be positive")
        if not 1 <= border_count <= ops.GBDT_MAX_BORDERS:
            raise ValueError(f"border_count must be in [1, {ops.GBDT_MAX_BORDERS}] (got {border_count})")
        if metric_period < 1:
            raise ValueError("metric_period must be >= 1")
        if one_hot_max_size is not None and not 1 <= one_hot_max_size <= _MAX_CODES:
            raise ValueError(f"one_hot_max_size must be None or in [1, {_MAX_CODES}] (got {one_hot_max_size})")
        p, a = (float(v) for v in ts_prior)
        if not (0.0 <= p <= 1.0 and a > 0 and math.isfinite(a)):
            raise ValueError(f"ts_prior must be (p in [0, 1], a > 0) (got {ts_prior})")
        if not 0 <= ts_seed < 2 ** 63:
            raise ValueError(f"ts_seed must be in [0, 2^63) (got {ts_seed})")
        self.one_hot_max_size = None if one_hot_max_size is None else int(one_hot_max_size)
        self.ts_prior, self.ts_seed = (p, a), int(ts_seed)
        self.iterations, self.learning_rate, self.depth = int(iterations), float(learning_rate), int(depth)
        self.l2_leaf_reg, self.border_count = float(l2_leaf_reg), int(border_count)
        self.cat_features = list(cat_features) if cat_features is not None else []
        self.early_stopping_rounds, self.metric_period = early_stopping_rounds, int(metric_period)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.model_, self._fitted_names = None, None
        self.leaf_weights_, self._explain_plan = None, None
        self._no_ts()
        self.tree_count_ = 0
        self.evals_result_, self.best_iteration_, self.best_score_ = None, None, None

    def _no_ts(self):
        """The state of a model without target-statistic columns. ts_cols_: the positions, among the categorical
        columns, of the TS columns; per TS column ts_table_ fp32 [V + 1], ts_totals_ int32 [V + 1, 2] = (N_c,
        S_c) and ts_bins_ uint8 [V + 1] = the table's bins under ts_borders_ / ts_n_borders_."""
        self.ts_cols_, self.ts_table_, self.ts_totals_, self.ts_bins_ = [], [], [], []
        self.ts_borders_, self.ts_n_borders_ = None, None

    # ---- columns -> bins ---------------------------------------------------------------------------
    def _split_columns(self, X):
        """(numeric fp32 [Fn, R] device tensor or None, categorical: a list of host value lists (vocabulary
        path) or an integer [Fc, R] device tensor of codes, or None, numeric names, categorical names)."""
        dev = self.device
        if isinstance(X, dict) or _is_frame(X):
            names = list(X.keys()) if isinstance(X, dict) else list(X.columns)
            cats = [n for i, n in enumerate(names) if n in self.cat_features or i in self.cat_features]
            nums = [n for n in names if n not in cats]
            if self.model_ is not None and self._fitted_names is not None:
                nums, cats = self._fitted_names      # predict: the training columns, by name
            num = None
            if nums:
                cols = [np.asarray(X[n], dtype=np.float32) for n in nums]
                num = torch.from_numpy(np.stack(cols)).to(dev)
            cat = [list(np.asarray(X[n], dtype=object)) for n in cats] if cats else None
            return num, cat, nums, cats
        if not isinstance(X, (tuple, list)) or len(X) != 2:
            raise TypeError("X must be a dict or DataFrame of columns, or a pair (numeric [R, Fn], categorical [R, Fc])")
        num, cat = X
        if num is not None:
            num = torch.as_tensor(num).to(dev, torch.float32)
            if num.dim() != 2:
                raise ValueError(f"the numeric block must be [R, Fn] (got {tuple(num.shape)})")
            num = num.t().contiguous()
        if cat is not None:
            cat = torch.as_tensor(cat)
            if cat.dim() != 2 or cat.dtype not in (torch.uint8, torch.int8, torch.int16, torch.int32, torch.int64):
                raise ValueError("the categorical block must be an integer [R, Fc] tensor")
            cat = cat.to(dev, torch.int64).t().contiguous()
        nums = [f"num{i}" for i in range(0 if num is None else num.shape[0])]
        cats = [f"cat{i}" for i in range(0 if cat is None else cat.shape[0])]
        return num, cat, nums, cats

    def _bins(self, X):
        """The uint8 [F, R] bins of X under the fitted borders and vocabularies (no host read)."""
        num, cat, nums, cats = self._split_columns(X)
        Fn, Fc = len(nums), len(cats)
        if (Fn, Fc) != (len(self._fitted_names[0]), len(self._fitted_names[1])):
            raise ValueError(f"X has {Fn} numeric and {Fc} categorical columns, the model was fitted on "
                             f"{len(self._fitted_names[0])} and {len(self._fitted_names[1])}")
        R = num.shape[1] if num is not None else (cat.shape[1] if torch.is_tensor(cat) else len(cat[0]))
        bins = torch.empty(Fn + Fc, R, device=self.device, dtype=torch.uint8)
        if Fn:
            ops.gbdt_bin(num, self.borders_, self.n_borders_, out=bins)
        if Fc and not self.ts_cols_:
            bins[Fn:] = self._codes(cat, R)
        elif Fc:
            self._cat_bins(self._wide_codes(cat, R), bins, Fn)
        return bins

    def _cat_rows(self, Fn, Fc):
        """The row of bins each categorical column has: the numeric columns, then the TS columns, then the
        one-hot ones, each kind in the caller's order."""
        oh = [k for k in range(Fc) if k not in self.ts_cols_]
        rows = {k: Fn + j for j, k in enumerate(self.ts_cols_)}
        rows.update({k: Fn + len(self.ts_cols_) + j for j, k in enumerate(oh)})
        return [rows[k] for k in range(Fc)]

    def _cat_bins(self, codes, bins, Fn):
        """bins rows Fn.. of served rows from codes int64 [Fc, R]: a TS column gathers its byte table (a code
        outside [0, V] reads entry 0), a one-hot column is its code (outside [0, 255]: 0)."""
        for k, row in enumerate(self._cat_rows(Fn, codes.shape[0])):
            c = codes[k]
            if k in self.ts_cols_:
                bins[row] = self._ts_bins_of(k, c)
            else:
                bins[row] = torch.where((c < 0) | (c > _MAX_CODES), torch.zeros_like(c), c).to(torch.uint8)

    def _ts_bins_of(self, k, c):
        """The bins uint8 of the codes c (int64, any shape) of categorical column k, a TS column: one gather of
        its byte table."""
        table = self.ts_bins_[self.ts_cols_.index(k)]
        return table[torch.where((c < 0) | (c >= table.numel()), torch.zeros_like(c), c)]

    def _wide_codes(self, cat, R):
        """The codes int64 [Fc, R] on the device: the tensor's own, or the vocabularies' (0 = unseen)."""
        if torch.is_tensor(cat):
            return cat
        host = np.empty((len(cat), R), np.int64)
        for k, (vals, vocab) in enumerate(zip(cat, self.vocab_)):
            host[k] = [vocab.get(v, 0) for v in vals]
        return torch.from_numpy(host).to(self.device)

    def _codes(self, cat, R):
        if torch.is_tensor(cat):
            return torch.where((cat < 0) | (cat > _MAX_CODES), torch.zeros_like(cat), cat).to(torch.uint8)
        host = np.empty((len(cat), R), np.uint8)
        for k, (vals, vocab) in enumerate(zip(cat, self.vocab_)):
            host[k] = [vocab.get(v, 0) for v in vals]
        return torch.from_numpy(host).to(self.device)

    # ---- training ----------------------------------------------------------------------------------
    def _fit_columns(self, X, y, check_labels):
        """The start of a fit: the columns of X split, the vocabularies, borders and n_bins_ built and the
        training rows binned. One host read (the label counts, with the largest code of tensor-given
        categorical columns in the same copy); check_labels(n_pos, n_neg) raises for labels the objective
        cannot train on. Returns (bins uint8 [F, R], y fp32 [R], is_cat uint8 [F], n_pos)."""
        dev = self.device
        self.model_, self._fitted_names = None, None
        self.leaf_weights_, self._explain_plan = None, None
        num, cat, nums, cats = self._split_columns(X)
        Fn, Fc = len(nums), len(cats)
        F = Fn + Fc
        if not 1 <= F <= ops.GBDT_MAX_FEATURES:
            raise ValueError(f"need between 1 and {ops.GBDT_MAX_FEATURES} columns (got {F})")
        y = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).to(dev, torch.float32).reshape(-1).contiguous()
        R = y.numel()
        stats = [(y == 1).sum(), (y == 0).sum()]
        self.vocab_ = []
        self._no_ts()
        ohm, known = self.one_hot_max_size, []      # known: the known values of every categorical column
        if Fc and torch.is_tensor(cat):
            stats += [cat.max(), cat.min()] + list(cat.max(dim=1).values)
        elif Fc:
            for name, vals in zip(cats, cat):
                vocab = {}
                for v in vals:
                    if v not in vocab:
                        vocab[v] = len(vocab) + 1
                if ohm is None and len(vocab) > _MAX_CODES:
                    raise ValueError(f"categorical column {name!r} has {len(vocab)} distinct values: at most "
                                     f"{_MAX_CODES} are supported (no target-statistic encoding)")
                self.vocab_.append(vocab)
                known.append(len(vocab))
        for name, block in (("numeric", num), ("categorical", cat)):
            n = None if block is None else (block.shape[1] if torch.is_tensor(block) else len(block[0]))
            if n is not None and n != R:
                raise ValueError(f"the {name} columns hold {n} rows for {R} labels")
        host = [int(v) for v in torch.stack([s.to(torch.int64) for s in stats]).tolist()]     # the one host read
        n_pos, n_neg = host[:2]
        if n_pos + n_neg != R:
            raise ValueError("labels must be 0 or 1")
        check_labels(n_pos, n_neg)
        if Fc and torch.is_tensor(cat):
            if ohm is None and (host[2] > _MAX_CODES or host[3] < 0):
                raise ValueError(f"categorical codes must be in [0, {_MAX_CODES}] (got {host[3]} .. {host[2]}): at most "
                                 f"{_MAX_CODES} known values besides 0 = unknown")
            if host[3] < 0:
                raise ValueError(f"categorical codes must be >= 0 (got {host[3]})")
            known = host[4:]
        if ohm is not None:
            self.ts_cols_ = [k for k, n in enumerate(known) if n > ohm]
            for k in self.ts_cols_:
                if known[k] > ops.GBDT_TS_MAX_CODES:
                    raise ValueError(f"categorical column {cats[k]!r} has {known[k]} known values: a target-statistic "
                                     f"column takes up to {ops.GBDT_TS_MAX_CODES}")
        Fts = len(self.ts_cols_)
        one_hot = [k for k in range(Fc) if k not in self.ts_cols_]
        n_bins = [self.border_count + 1] * (Fn + Fts) + [known[k] + 1 for k in one_hot]
        self._fitted_names = (nums, cats)
        self.feature_names_ = nums + cats
        if Fn:
            self.borders_, self.n_borders_ = build_borders(num, self.border_count)
        else:
            self.borders_, self.n_borders_ = None, None
        is_cat = torch.tensor([0] * (Fn + Fts) + [1] * len(one_hot), dtype=torch.uint8, device=dev)
        self.n_bins_ = torch.tensor(n_bins, dtype=torch.int32, device=dev)
        bins = torch.empty(F, R, device=dev, dtype=torch.uint8)
        if Fn:
            ops.gbdt_bin(num, self.borders_, self.n_borders_, out=bins)
        if Fc and not Fts:
            bins[Fn:] = self._codes(cat, R)
        elif Fc:
            codes = self._wide_codes(cat, R)
            self._fit_ts(codes, y, [known[k] for k in self.ts_cols_], bins[Fn:])
            if one_hot:
                bins[Fn + Fts:] = codes[one_hot].to(torch.uint8)      # in [0, one_hot_max_size]: checked above
        return bins, y, is_cat, n_pos

    def _fit_ts(self, codes, y, V, out):
        """The TS columns of a fit: codes int64 [Fc, R] -> the ordered training values (ops.gbdt_ts_plan,
        ops.gbdt_ordered_ts), their borders and bins (rows 0..Fts-1 of out), and per column the table, the
        totals and the byte table the served rows gather. V: the columns' known values. No host read."""
        ts_codes = codes[self.ts_cols_].to(torch.int32).contiguous()
        order = ops.gbdt_ts_plan(ts_codes, self.ts_seed)
        ts, totals, table = ops.gbdt_ordered_ts(ts_codes, order, y, V, self.ts_prior)
        self.ts_borders_, self.ts_n_borders_ = build_borders(ts, self.border_count)
        ops.gbdt_bin(ts, self.ts_borders_, self.ts_n_borders_, out=out)
        table_bins = ops.gbdt_bin(table, self.ts_borders_, self.ts_n_borders_)
        self.ts_table_ = [table[j, :v + 1].clone() for j, v in enumerate(V)]
        self.ts_totals_ = [totals[j, :v + 1].clone() for j, v in enumerate(V)]
        self.ts_bins_ = [table_bins[j, :v + 1].clone() for j, v in enumerate(V)]

    def _new_model(self, is_cat, f0):
        """The empty GBDTModel of `iterations` trees a fit fills (model_)."""
        T, dev = self.iterations, self.device
        self.model_ = ops.GBDTModel(torch.zeros(T, ops.GBDT_MAX_DEPTH, 2, device=dev, dtype=torch.int32),
                                    torch.zeros(T, ops.GBDT_LEAF_STRIDE, device=dev, dtype=torch.float32), is_cat,
                                    self.depth, f0, 0)
        return self.model_

    # ---- prediction ----------------------------------------------------------------------------------
    def _fitted(self):
        if self.model_ is None:
            raise RuntimeError("the model is not fitted")
        return self.model_

    @torch.no_grad()
    def predict_logits(self, X, ntree_end=None):
        """The raw scores [R] (fp32 device tensor) of X after the first ntree_end trees (default: tree_count_):
        bit-identical to the training approximant after as many trees for a model without TS columns. With TS
        columns the training rows saw their ordered values and the rows given here read the table's, so on the
        training rows the two differ."""
        model = self._fitted()
        if ntree_end is not None and not 0 <= ntree_end <= model.splits.shape[0]:
            raise ValueError(f"ntree_end must be in [0, {model.splits.shape[0]}] (got {ntree_end})")
        return ops.gbdt_predict(self._bins(X), model, ntree_end=ntree_end)

    # ---- explanations ---------------------------------------------------------------------------------
    def _count_leaves(self, bins):
        """leaf_weights_ int64 [tree_count_, 64] = the rows of bins per leaf of the trees in use (no host read)."""
        model = self._fitted()
        self.leaf_weights_ = ops.gbdt_leaf_weights(bins, model)[:model.n_trees]
        self._explain_plan = None

    @torch.no_grad()
    def calc_leaf_weights(self, X):
        """Recompute leaf_weights_ from the rows X (as predict_logits takes them): what a model loaded from a
        file without weights needs before it can explain itself, and a way to explain a model against other
        rows than its training set. Returns self."""
        self._count_leaves(self._bins(X))
        return self

    def _plan(self):
        self._fitted()
        if self.leaf_weights_ is None:
            raise RuntimeError("the model has no leaf weights (it was loaded from a file written before they were "
                               "saved): call calc_leaf_weights(X) first")
        if self._explain_plan is None:
            self._explain_plan = ops.gbdt_explain_plan(self.model_, self.leaf_weights_)
        return self._explain_plan

    def _name_order(self):
        """The internal column (numeric, target-statistic, one-hot) of every entry of feature_names_."""
        Fn, Fc = len(self._fitted_names[0]), len(self._fitted_names[1])
        return list(range(Fn)) + self._cat_rows(Fn, Fc)

    def _shap_of_bins(self, bins):
        """ShapValues float64 [R, F + 1] of binned rows: the transposed view of ops.gbdt_shap's [F + 1, R] (of a
        copy with the rows reordered where the model has target-statistic columns, whose internal order differs
        from feature_names_')."""
        phi = ops.gbdt_shap(bins, self.model_, self._plan())
        order = self._name_order()
        if order != list(range(len(order))):
            phi = phi.index_select(0, torch.tensor(order + [len(order)], device=phi.device))
        return phi.t()

    @torch.no_grad()
    def get_feature_importance(self, data=None, type="PredictionValuesChange", y=None, group_id=None):
        """CatBoost's get_feature_importance, in feature_names_ order.
        "PredictionValuesChange" (data not needed): a host float64 [F] summing to 100 (all zeros for a model
            whose trees never change a prediction): per tree and level the cover-weighted squared differences of
            the leaf pairs the level separates, from leaf_weights_; one host read, the per-feature sums formed on
            the host in tree order.
        "ShapValues": data (rows as predict_logits takes them) -> a device float64 [R, F + 1], exact
            path-dependent Shapley values of the raw score with the expected value last; a row sums to its raw
            score. No host read.
        "LossFunctionChange": data, y (and group_id for a ranker) -> a host float64 [F]: metric(F - phi_j) -
            metric(F) with the model's own loss (Logloss mean, QuerySoftMax), CatBoost's SHAP-based approximation;
            positive = the feature helps. F + 1 evaluations on the device (ops.binary_eval /
            ops.query_softmax_eval), fetched by one host read (a ranker's group plan reads the host once more).
        RuntimeError without leaf weights (calc_leaf_weights)."""
        model = self._fitted()
        if type == "PredictionValuesChange":
            plan = self._plan()
            n, depth = model.n_trees, model.depth
            host = torch.cat([plan.pvc[:n, :depth].reshape(-1),
                              model.splits[:n, :depth, 0].reshape(-1).to(torch.float64)]).cpu().numpy()     # the one host read
            pvc, feat = host[:n * depth], host[n * depth:].astype(np.int64)
            F = len(self.feature_names_)
            feat = np.where((feat < 0) | (feat >= F), 0, feat)
            imp = np.zeros(F, np.float64)
            for v, f in zip(pvc, feat):       # tree order, level by level
                imp[f] += v
            total = imp.sum()
            imp = imp * (100.0 / total) if total > 0 else imp
            return imp[self._name_order()]
        if type not in ("ShapValues", "LossFunctionChange"):
            raise ValueError(f'type must be "PredictionValuesChange", "ShapValues" or "LossFunctionChange" (got {type!r})')
        if data is None:
            raise ValueError(f"{type} needs data")
        self._plan()
        bins = self._bins(data)
        phi = self._shap_of_bins(bins)
        if type == "ShapValues":
            return phi
        if y is None:
            raise ValueError("LossFunctionChange needs y")
        R, F = phi.shape[0], phi.shape[1] - 1
        y = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).to(self.device, torch.float32).reshape(-1).contiguous()
        if y.numel() != R:
            raise ValueError(f"y holds {y.numel()} labels for {R} rows")
        raw = ops.gbdt_predict(bins, model)
        without = [(raw.double() - phi[:, j]).float() for j in range(F)]
        return self._loss_change(raw, without, y, group_id)

    @property
    def feature_importances_(self):
        return self.get_feature_importance()

    # ---- persistence -----------------------------------------------------------------------------------
    def save_model(self, path):
        """torch.save of the trees in use, the borders and the vocabularies, under the class's loss_function:
        format "oblivious_gbdt/1", or with TS columns "oblivious_gbdt/2", which adds their positions, tables,
        totals, borders and byte tables and the three TS parameters."""
        m = self._fitted()
        n = m.n_trees
        cpu = lambda t: None if t is None else t.detach().cpu()   # noqa: E731
        sd = {"format": "oblivious_gbdt/1", "loss_function": self.loss_function, "splits": cpu(m.splits[:n]), "leaf_values": cpu(m.leaf_values[:n]),
              "is_cat": cpu(m.is_cat), "depth": m.depth, "f0": m.f0, "borders": cpu(self.borders_),
              "n_borders": cpu(self.n_borders_), "n_bins": cpu(self.n_bins_), "vocab": self.vocab_,
              "names": self._fitted_names,
              "params": {"iterations": self.iterations, "learning_rate": self.learning_rate, "depth": self.depth,
                         "l2_leaf_reg": self.l2_leaf_reg, "border_count": self.border_count,
                         "cat_features": self.cat_features},
              "best_iteration": self.best_iteration_, "best_score": self.best_score_,
              "evals_result": self.evals_result_, "leaf_weights": cpu(self.leaf_weights_)}
        if self.ts_cols_:
            sd["format"] = "oblivious_gbdt/2"
            sd["params"].update(one_hot_max_size=self.one_hot_max_size, ts_prior=self.ts_prior, ts_seed=self.ts_seed)
            sd["ts"] = {"cols": list(self.ts_cols_), "table": [cpu(t) for t in self.ts_table_],
                        "totals": [cpu(t) for t in self.ts_totals_], "bins": [cpu(t) for t in self.ts_bins_],
                        "borders": cpu(self.ts_borders_), "n_borders": cpu(self.ts_n_borders_)}
        torch.save(sd, path)

    def load_model(self, path):
        sd = torch.load(path, map_location="cpu", weights_only=False)
        if sd.get("format") not in ("oblivious_gbdt/1", "oblivious_gbdt/2"):
            raise ValueError(f"{path} is not an ObliviousBoostingClassifier model")
        loss = sd.get("loss_function", "Logloss")      # files written before the ranker existed carry no key
        if loss != self.loss_function:
            raise ValueError(f"{path} holds a {loss} model: {type(self).__name__} loads {self.loss_function} models")
        dev = self.device
        to = lambda t: None if t is None else t.to(dev).contiguous()   # noqa: E731
        for k, v in sd["params"].items():
            setattr(self, k, v)
        self.model_ = ops.GBDTModel(to(sd["splits"]), to(sd["leaf_values"]), to(sd["is_cat"]), sd["depth"], sd["f0"],
                                    sd["splits"].shape[0])
        self.borders_, self.n_borders_, self.n_bins_ = to(sd["borders"]), to(sd["n_borders"]), to(sd["n_bins"])
        self.vocab_, self._fitted_names = sd["vocab"], tuple(sd["names"])
        self._no_ts()
        if sd["format"] == "oblivious_gbdt/2":
            ts = sd["ts"]
            self.ts_cols_ = list(ts["cols"])
            self.ts_table_, self.ts_totals_, self.ts_bins_ = ([to(t) for t in ts[k]] for k in ("table", "totals", "bins"))
            self.ts_borders_, self.ts_n_borders_ = to(ts["borders"]), to(ts["n_borders"])
        self.feature_names_ = list(self._fitted_names[0]) + list(self._fitted_names[1])
        self.best_iteration_, self.best_score_, self.evals_result_ = sd["best_iteration"], sd["best_score"], sd["evals_result"]
        self.tree_count_ = self.model_.n_trees
        self.leaf_weights_, self._explain_plan = to(sd.get("leaf_weights")), None      # None: a file from before the weights
        return self


class ObliviousBoostingClassifier(_ObliviousBoosting):
    """Binary classifier of `iterations` oblivious trees of `depth` <= 6 levels boosted on Logloss.

    X is a dict or DataFrame of columns (those named in cat_features are categorical: any hashable
    values, coded by a vocabulary built from the training rows, code 0 = unseen; at most 255 distinct
    values; the others numeric), or a pair (numeric [R, Fn] float, categorical [R, Fc] integer) of tensors
    or arrays, either may be None; there the categorical values are codes already, in [0, 255] (a value
    outside it predicts as 0). Internally the numeric columns come first, then the categorical ones: that
    is the order in which ties between equally good splits are broken.

    one_hot_max_size=n in [1, 255] (default None: every categorical column one-hot, as above) makes a
    categorical column with more than n known values (the vocabulary's size, or the largest code of a tensor
    column) a target-statistic column of up to ops.GBDT_TS_MAX_CODES known values: its training rows carry the
    ordered statistic (s_i + a p) / (n_i + a) over the rows of the same code that precede them in the order
    hash_u32(ts_seed + TS column index, row), ts_prior = (p, a); validation and served rows read the table of
    the totals, through a byte table per column (ts_bins_), and a code outside [0, V] reads entry 0. Such a
    column is numeric from there on (borders of the ordered values, is_cat 0). The internal order is then
    numeric, TS, one-hot columns, each kind in the caller's order: the tie-break order. predict_logits on the
    training rows no longer equals the training approximant of such a model.

    After fit: tree_count_, feature_names_, leaf_weights_ (int64 [tree_count_, 64] on the device: the training rows
    per leaf, what get_feature_importance and feature_importances_ explain the model with), and with an eval_set
    evals_result_, best_iteration_ (the 0-based index of the best tree) and best_score_, as DeepFM.fit fills them."""

    loss_function = "Logloss"

    @torch.no_grad()
    def fit(self, X, y, eval_set=None, eval_metric="AUC", use_best_model=None, eval_group_id=None,
            record_approximants=()):
        """Boost `iterations` trees on X / y [R] in {0, 1}. Nothing synchronises with the host inside a tree
        and the splits stay on the device; a plain fit reads the host once (the label counts, with the largest
        code of tensor-given categorical columns in the same copy).

        eval_set=(X_val, y_val) adds the reference's validation (:98-108, :123-135) with the semantics
        DeepFM.fit documents: after every metric_period-th tree (and the last) the validation scores are
        advanced by the new trees and evaluated on the device (ops.binary_eval; with eval_group_id also
        ops.group_eval), one host read per evaluation that also carries the training Logloss after that tree.
        eval_metric "AUC", "Logloss", "NDCG", "NDCG:top=K" or "QueryAUC" picks the best evaluation (only a
        strictly better one replaces it), early_stopping_rounds (the constructor's) stops after that many
        evaluations without an improvement, and use_best_model (default True with an eval_set) truncates the
        model to best_iteration_ + 1 trees. record_approximants: tree counts t after which the training
        approximant is kept (approximants_[t], a device tensor), for tests."""
        esr = self.early_stopping_rounds if eval_set is not None else None
        use_best_model = _fit_args(eval_set, eval_metric, esr, use_best_model, None, eval_group_id)
        metric, top = _parse_eval_metric(eval_metric)
        dev = self.device

        def two_classes(n_pos, n_neg):
            if n_pos == 0 or n_neg == 0:
                raise ValueError("the training labels hold a single class")

        bins, y, is_cat, n_pos = self._fit_columns(X, y, two_classes)
        F, R = bins.shape
        f0 = float(np.float32(math.log(n_pos / R / (1.0 - n_pos / R))))
        T = self.iterations
        model = self._new_model(is_cat, f0)

        validate = eval_set is not None
        if validate:
            Xv, yv = eval_set
            yv = torch.as_tensor(np.asarray(yv) if not torch.is_tensor(yv) else yv).to(dev, torch.float32).reshape(-1)
            yv = yv.contiguous()
            _fit_eval_labels(yv, eval_metric)
            gv = None if eval_group_id is None else _fit_eval_groups(yv, eval_group_id, eval_metric)
            bins_v = self._bins(Xv)
            if bins_v.shape[1] != yv.numel():
                raise ValueError(f"eval_set has {bins_v.shape[1]} rows for {yv.numel()} labels")
            Fv = torch.full((yv.numel(),), f0, device=dev, dtype=torch.float32)
            self.evals_result_ = {"learn": {"Logloss": []}, "validation": {"Logloss": [], "AUC": []}}
            self.best_iteration_, self.best_score_ = None, None
        best, since, scored = None, 0, 0

        Fx = torch.full((R,), f0, device=dev, dtype=torch.float32)
        scratch = ops.GBDTScratch(R, F, self.depth, dev)
        keep = set(int(t) for t in record_approximants)
        self.approximants_ = {}
        built = 0
        for t in range(T):
            ops.gbdt_tree(bins, y, Fx, is_cat, self.n_bins_, self.depth, self.learning_rate, self.l2_leaf_reg,
                          model.splits[t], model.leaf_values[t], scratch)
            built = t + 1
            if built in keep:
                self.approximants_[built] = Fx.clone()
            if not validate or (built % self.metric_period != 0 and built != T):
                continue
            ops.gbdt_predict(bins_v, model, ntree_begin=scored, ntree_end=built, init=Fv, out=Fv)
            scored = built
            learn = ops.binary_eval(Fx, y).loss_sum / R
            be = ops.binary_eval(Fv, yv)
            if gv is None:
                res, (learn,) = be.result(also=learn)
                now = {"Logloss": res["logloss"], "AUC": res["auc"]}
            else:
                res, grp, (learn,) = ops._fetch_evals(be, ops.group_eval(Fv, yv, gv, top=top), also=learn)
                now = {"Logloss": res["logloss"], "AUC": res["auc"], "NDCG": grp["ndcg"], "QueryAUC": grp["query_auc"]}
            ev = self.evals_result_
            ev["learn"]["Logloss"].append(learn)
            for name, value in now.items():
                ev["validation"].setdefault(name, []).append(value)
            score = -now["Logloss"] if metric == "Logloss" else now[metric]
            if best is None or score > best:
                best, since = score, 0
                self.best_iteration_ = t
                self.best_score_ = {"validation": now}
            else:
                since += 1
            if esr is not None and since >= esr:
                break
        ops._GBDT_GUARD.watch(scratch.flag)      # a range error is reported by the next gbdt call, or by check()
        model.n_trees = self.best_iteration_ + 1 if (validate and use_best_model) else built
        self.tree_count_ = model.n_trees
        self._count_leaves(bins)
        return self

    def _loss_change(self, raw, without, y, group_id):
        """LossFunctionChange: the Logloss mean of every score vector of `without` minus that of raw."""
        R = raw.numel()
        base = ops.binary_eval(raw, y)
        _, sums = base.result(also=torch.cat([base.loss_sum] + [ops.binary_eval(z, y).loss_sum for z in without]))
        return (np.asarray(sums[1:], np.float64) - sums[0]) / R

    def predict_proba(self, X) -> np.ndarray:
        """CatBoost's shape: [R, 2] = (1 - p, p) with p = sigmoid(raw score), a host array."""
        p = torch.sigmoid(self.predict_logits(X))
        return torch.stack([1.0 - p, p], dim=1).cpu().numpy()


def _parse_rank_metric(eval_metric):
    """A ranker's eval_metric -> (the key of evals_result_["validation"] it selects, the NDCG cut-off):
    "QuerySoftMax" (smaller is better), "NDCG", "NDCG:top=K" or "QueryAUC"."""
    if eval_metric == "QuerySoftMax":
        return "QuerySoftMax", 10
    if eval_metric in ("AUC", "Logloss"):
        raise ValueError(f'a ranker\'s eval_metric must be "QuerySoftMax", "NDCG", "NDCG:top=K" or "QueryAUC" '
                         f"(got {eval_metric!r})")
    return _parse_eval_metric(eval_metric)


class ObliviousBoostingRanker(_ObliviousBoosting):
    """Ranker of `iterations` oblivious trees boosted on QuerySoftMax, the group-normalised softmax loss
    (include/recsys_amd.h, "QuerySoftMax"; restated by tests/gbdt_rank_ref.py): the rows carry y in {0, 1}
    and a group id (the reference's per-customer ranker rows, utils/monitor/log_importer.py), and every
    group with a positive weighs the same. X as ObliviousBoostingClassifier's; the base score is 0. The
    trees, the histograms and the prediction are the classifier's: only the gradient stage differs
    (ops.gbdt_tree(groups=...)). Every sum is an integer sum and every group reduction is order-free: two
    fits give the same model bit for bit, and so does a fit on the same rows in another order. With TS columns
    (one_hot_max_size) the statistics are computed on the caller's row order, before the permutation into
    group order, and depend on it: the second property then holds only for a model without TS columns."""

    loss_function = "QuerySoftMax"

    @torch.no_grad()
    def fit(self, X, y, group_id, eval_set=None, eval_group_id=None, eval_metric="NDCG:top=10", use_best_model=None,
            record_approximants=()):
        """Boost `iterations` trees on X / y [R] in {0, 1} / group_id [R] (int32 or int64 ids >= 0, the rows of a
        group anywhere). The bins and labels are permuted into group order once (ops.GBDTGroupPlan); nothing
        synchronises with the host inside a tree. A plain fit reads the host twice (the plan's number of
        groups, the label counts). ValueError when no group holds a positive.

        eval_set=(X_val, y_val) with eval_group_id [validation rows] validates as the classifier does: after
        every metric_period-th tree (and the last) the validation scores are advanced by the new trees and
        evaluated on the device, one host read per evaluation: evals_result_["learn"]["QuerySoftMax"] (the
        training loss after that tree) and evals_result_["validation"]["QuerySoftMax" | "NDCG" | "QueryAUC"]
        (ops.query_softmax_eval, ops.group_eval). eval_metric "QuerySoftMax" (smaller is better), "NDCG",
        "NDCG:top=K" or "QueryAUC" picks the best evaluation; early_stopping_rounds, best_iteration_,
        best_score_ and use_best_model as ObliviousBoostingClassifier.fit. record_approximants: tree counts t
        after which the training approximant is kept (approximants_[t], in group order: the rows
        [group_plan_.order]), for tests."""
        metric, top = _parse_rank_metric(eval_metric)
        validate = eval_set is not None
        if not validate:
            if eval_group_id is not None:
                raise ValueError("eval_group_id needs an eval_set")
            if use_best_model:
                raise ValueError("use_best_model needs an eval_set")
            use_best_model = False
        else:
            if eval_group_id is None:
                raise ValueError("a ranker's eval_set needs eval_group_id")
            if self.early_stopping_rounds is not None and self.early_stopping_rounds < 1:
                raise ValueError("early_stopping_rounds must be >= 1")
            use_best_model = True if use_best_model is None else use_best_model
        esr = self.early_stopping_rounds if validate else None
        dev = self.device

        def a_positive(n_pos, n_neg):
            if n_pos == 0:
                raise ValueError("no group holds a positive: QuerySoftMax has nothing to train on")

        bins, y, is_cat, _ = self._fit_columns(X, y, a_positive)
        F, R = bins.shape
        if len(group_id) != R:
            raise ValueError(f"group_id has {len(group_id)} ids for {R} rows")
        plan = self.group_plan_ = ops.GBDTGroupPlan(group_id, dev)
        bins = bins.index_select(1, plan.order).contiguous()      # group order, once
        y = y.index_select(0, plan.order).contiguous()
        T = self.iterations
        model = self._new_model(is_cat, 0.0)

        if validate:
            Xv, yv = eval_set
            yv = torch.as_tensor(np.asarray(yv) if not torch.is_tensor(yv) else yv).to(dev, torch.float32).reshape(-1)
            yv = yv.contiguous()
            _fit_eval_labels(yv, eval_metric)
            gv = _fit_eval_groups(yv, eval_group_id, "NDCG" if metric == "QuerySoftMax" else eval_metric)
            bins_v = self._bins(Xv)
            if bins_v.shape[1] != yv.numel():
                raise ValueError(f"eval_set has {bins_v.shape[1]} rows for {yv.numel()} labels")
            plan_v = ops.GBDTGroupPlan(gv, dev)
            yv_grouped = yv.index_select(0, plan_v.order).contiguous()
            Fv = torch.zeros(yv.numel(), device=dev, dtype=torch.float32)
            self.evals_result_ = {"learn": {"QuerySoftMax": []},
                                  "validation": {"QuerySoftMax": [], "NDCG": [], "QueryAUC": []}}
            self.best_iteration_, self.best_score_ = None, None
        best, since, scored = None, 0, 0

        Fx = torch.zeros(R, device=dev, dtype=torch.float32)
        scratch = ops.GBDTScratch(R, F, self.depth, dev)
        keep = set(int(t) for t in record_approximants)
        self.approximants_ = {}
        built = 0
        for t in range(T):
            ops.gbdt_tree(bins, y, Fx, is_cat, self.n_bins_, self.depth, self.learning_rate, self.l2_leaf_reg,
                          model.splits[t], model.leaf_values[t], scratch, groups=plan)
            built = t + 1
            if built in keep:
                self.approximants_[built] = Fx.clone()
            if not validate or (built % self.metric_period != 0 and built != T):
                continue
            ops.gbdt_predict(bins_v, model, ntree_begin=scored, ntree_end=built, init=Fv, out=Fv)
            scored = built
            learn = ops.query_softmax_eval(Fx, y, plan)
            val = ops.query_softmax_eval(Fv.index_select(0, plan_v.order), yv_grouped, plan_v)
            grp = ops.group_eval(Fv, yv, gv, top=top)
            host = torch.cat([learn._buf, val._buf, grp._buf]).cpu()      # the one host read
            grp = grp._result(host[4:10])
            now = {"QuerySoftMax": val._result(host[2:4])["loss"], "NDCG": grp["ndcg"], "QueryAUC": grp["query_auc"]}
            ev = self.evals_result_
            ev["learn"]["QuerySoftMax"].append(learn._result(host[:2])["loss"])
            for name, value in now.items():
                ev["validation"][name].append(value)
            score = -now["QuerySoftMax"] if metric == "QuerySoftMax" else now[metric]
            if best is None or score > best:
                best, since = score, 0
                self.best_iteration_ = t
                self.best_score_ = {"validation": now}
            else:
                since += 1
            if esr is not None and since >= esr:
                break
        ops._GBDT_GUARD.watch(scratch.flag)      # a range error is reported by the next gbdt call, or by check()
        model.n_trees = self.best_iteration_ + 1 if (validate and use_best_model) else built
        self.tree_count_ = model.n_trees
        self._count_leaves(bins)
        return self

    def _loss_change(self, raw, without, y, group_id):
        """LossFunctionChange: the QuerySoftMax of every score vector of `without` minus that of raw."""
        if group_id is None:
            raise ValueError("a ranker's LossFunctionChange needs group_id")
        if len(group_id) != raw.numel():
            raise ValueError(f"group_id has {len(group_id)} ids for {raw.numel()} rows")
        plan = ops.GBDTGroupPlan(group_id, self.device)
        yg = y.index_select(0, plan.order).contiguous()
        evals = [ops.query_softmax_eval(z.index_select(0, plan.order).contiguous(), yg, plan) for z in [raw] + without]
        host = torch.cat([e._buf for e in evals]).cpu()      # the one host read
        loss = [ops.QuerySoftMaxEval._result(host[2 * i:2 * i + 2])["loss"] for i in range(len(evals))]
        return np.asarray(loss[1:], np.float64) - loss[0]

    def predict(self, X, ntree_end=None):
        """The raw scores [R] (fp32 device tensor, the rows in X's order) after the first ntree_end trees
        (default: tree_count_): what orders the rows of a group. predict_logits under CatBoost's name."""
        return self.predict_logits(X, ntree_end)
