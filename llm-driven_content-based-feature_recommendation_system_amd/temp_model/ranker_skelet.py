"""Drop-in for temp_model/ranker_skelet.py: retrieval -> rerank.

Reference (temp_model/ranker_skelet.py):
  * FeatureEngineer :13-89, RecommendationRanker (CatBoost) :95-149, ReRankingSystem :155-237
  * the neural ranker the north star asks for (DeepFM) does not exist in the reference; it
    is specified by deepctr-torch 0.2.9 (pinned in requirements.txt:41, never imported) and
    lives here as `DeepFM`, with a CatBoost-compatible `predict_proba` wrapper.
  * CrossNet :239-272 and RankingModel (DCN-V2) :274-357 — dead code in the reference, kept
    as a second neural reranker with the same parameter names and init.
Compute: DeepFM forward = rsx_deepfm_embed + rsx_linear_fwd + rsx_linear_dot_fwd; DeepFM training
(the reference trains its ranker before use, RecommendationRanker.train :114-137, Logloss) =
ops.deepfm_train_step (DeepFM.make_trainer / DeepFM.fit); its validation (eval_set, eval_metric='AUC',
early_stopping_rounds, use_best_model, :98-108 and :123-135) = DeepFM.evaluate / DeepFM.fit(eval_set=...)
over ops.binary_eval (rsx_binary_eval: exact tie-aware AUC and Logloss on the device) and, for rows
that carry the per-customer group id of the reference's ranker data (utils/monitor/log_importer.py),
ops.group_eval (rsx_group_eval: per-query NDCG@top and QueryAUC; evaluate(group_id=...),
fit(eval_group_id=..., eval_metric="NDCG" | "NDCG:top=K" | "QueryAUC")); retrieval
(user_vec @ item_vectors.T -> topk, :193-196) = rsx_retrieve_topk (see ops.retrieve_topk). The
boosted-tree ranker itself (RecommendationRanker, :95-149) runs on the device as backend "native":
oblivious_gbdt.ObliviousBoostingClassifier (rsx_gbdt_*), served in batches through rsx_rerank_tabular; with
loss_function "QuerySoftMax" it is oblivious_gbdt.ObliviousBoostingRanker, trained on the rows' group ids
(rsx_gbdt_tree_grouped) and served by its raw score. RecommendationRanker.train_rows fits either from rows that
stay on the device (utils/monitor/log_importer.py: HMLogImporter.load_rows; ReRankingSystem.training_rows), with
the columns of rsx_pair_tabular, whose arithmetic is rsx_rerank_tabular's.
"""
from __future__ import annotations

from typing import Dict, List

import numpy as np
import torch
import torch.nn as nn

from .. import ops


def _parse_eval_metric(eval_metric):
    """eval_metric -> (the key of evals_result_["validation"] it selects, the NDCG cut-off): "AUC",
    "Logloss", "QueryAUC", "NDCG" (top 10) or "NDCG:top=K"."""
    if eval_metric in ("AUC", "Logloss", "QueryAUC", "NDCG"):
        return eval_metric, 10
    if isinstance(eval_metric, str) and eval_metric.startswith("NDCG:"):
        suffix = eval_metric[len("NDCG:"):]
        digits = suffix[len("top="):]
        if not suffix.startswith("top=") or not (digits.isascii() and digits.isdigit()):
            raise ValueError(f'eval_metric "NDCG" takes the suffix ":top=K" with an integer K (got {eval_metric!r})')
        top = int(digits)
        if not 1 <= top <= ops.NDCG_MAX_TOP:
            raise ValueError(f"eval_metric {eval_metric!r}: top must be in [1, {ops.NDCG_MAX_TOP}]")
        return "NDCG", top
    raise ValueError('eval_metric must be "AUC", "Logloss", "NDCG", "NDCG:top=K" or "QueryAUC" '
                     f"(got {eval_metric!r})")


def _fit_args(eval_set, eval_metric, early_stopping_rounds, use_best_model, eval_every, eval_group_id=None):
    """The argument checks of fit (DeepFM.fit documents them) that need no data; returns the
    effective use_best_model (default True with an eval_set)."""
    metric, _ = _parse_eval_metric(eval_metric)
    if metric in ("NDCG", "QueryAUC") and eval_group_id is None:
        raise ValueError(f"eval_metric {eval_metric!r} is a per-group metric: it needs eval_group_id")
    if eval_set is None:
        if eval_group_id is not None:
            raise ValueError("eval_group_id needs an eval_set")
        if early_stopping_rounds is not None or eval_every is not None or use_best_model:
            raise ValueError("early_stopping_rounds, eval_every and use_best_model need an eval_set")
        return False
    if early_stopping_rounds is not None and early_stopping_rounds < 1:
        raise ValueError("early_stopping_rounds must be >= 1")
    if eval_every is not None and eval_every < 1:
        raise ValueError("eval_every must be >= 1")
    return True if use_best_model is None else use_best_model


def _fit_eval_labels(yv, eval_metric):
    """ValueError for validation labels outside {0, 1} or a single class with eval_metric "AUC" (one host read)."""
    n_pos, n_neg = (int(v) for v in torch.stack([(yv == 1).sum(), (yv == 0).sum()]).tolist())
    if n_pos + n_neg != yv.numel():
        raise ValueError("eval_set labels must be 0 or 1")
    if eval_metric == "AUC" and (n_pos == 0 or n_neg == 0):
        raise ValueError('eval_set holds a single class: eval_metric="AUC" is undefined')


def _fit_eval_groups(yv, eval_group_id, eval_metric):
    """eval_group_id as the int32 device tensor of the validation rows yv. ValueError for a wrong
    length, an id outside [0, 2^31), eval_metric "NDCG" with no group that holds a positive or
    "QueryAUC" with no group that holds both classes (one host read: ops.group_eval on zero logits)."""
    n = len(eval_group_id)
    if n != yv.numel():
        raise ValueError(f"eval_group_id has {n} ids for {yv.numel()} validation rows")
    gv = ops.group_ids_int32(eval_group_id, yv.device)
    metric, top = _parse_eval_metric(eval_metric)
    try:
        res = ops.group_eval(torch.zeros_like(yv), yv, gv, top=top).result()
    except ValueError as e:
        raise ValueError(f"eval_group_id: {e}") from None
    if metric == "NDCG" and res["ndcg_groups"] == 0:
        raise ValueError(f"no group of the eval_set holds a positive: eval_metric={eval_metric!r} is undefined")
    if metric == "QueryAUC" and res["auc_groups"] == 0:
        raise ValueError('no group of the eval_set holds both classes: eval_metric="QueryAUC" is undefined')
    return gv


def _evaluate_result(run, rows, y, batch_size, group_id, top):
    """The dict of evaluate: run = the model's _evaluate_on_device, rows = its row arguments. One host
    read with or without group_id."""
    if group_id is None:
        res = run(*rows, batch_size).result()
        return {"Logloss": res["logloss"], "AUC": res["auc"]}
    g = ops.group_ids_int32(group_id, y.device)
    if g.numel() != y.numel():
        raise ValueError(f"group_id has {g.numel()} ids for {y.numel()} rows")
    res, grp = ops._fetch_evals(*run(*rows, batch_size, g, top))
    return {"Logloss": res["logloss"], "AUC": res["auc"], "NDCG": grp["ndcg"], "QueryAUC": grp["query_auc"]}


def _fit_loop(model, tr, step, R, dev, batch_size, epochs, shuffle, seed, validate, eval_metric,
              early_stopping_rounds, use_best_model, eval_every, after_steps=None):
    """The training loop of DeepFM.fit and RankingModel.fit (semantics: DeepFM.fit's docstring).
    step(sel) -> the loss of the batch of rows sel (a slice, or an index tensor when shuffled);
    tr.reduction says how it was reduced. validate: None, or a callable returning the validation
    rows' ops.BinaryEval, or (with eval_group_id) their (ops.BinaryEval, ops.GroupEval). after_steps:
    called once the last step was taken, before the best parameters are restored. Returns the
    completed epochs' mean row losses."""
    gen = torch.Generator().manual_seed(seed)
    means = []
    if validate is None:
        for _ in range(epochs):
            order = torch.randperm(R, generator=gen).to(dev) if shuffle else None
            total = torch.zeros((), device=dev, dtype=torch.float64)
            for s in range(0, R, batch_size):
                e = min(R, s + batch_size)
                loss = step(slice(s, e) if order is None else order[s:e])
                total += loss * (e - s) if tr.reduction == "mean" else loss
            means.append(float((total / R).item()))
        if after_steps is not None:
            after_steps()
        return means

    model.evals_result_ = {"learn": {"Logloss": []}, "validation": {"Logloss": [], "AUC": []}}
    model.best_iteration_, model.best_score_ = None, None
    metric, _ = _parse_eval_metric(eval_metric)
    params = list(model.parameters())
    snapshot, stale = None, False      # stale: steps were taken since the snapshot was written
    state = {"best": None, "since": 0}

    def evaluate_now(learn_mean):
        """One evaluation; learn_mean: 0-d float64 device tensor. True when training should stop."""
        nonlocal snapshot, stale
        evs = validate()
        if isinstance(evs, tuple):      # with eval_group_id: both blocks and the learn mean in one copy
            res, grp, (learn,) = ops._fetch_evals(*evs, also=learn_mean)
            now = {"Logloss": res["logloss"], "AUC": res["auc"], "NDCG": grp["ndcg"], "QueryAUC": grp["query_auc"]}
        else:
            res, (learn,) = evs.result(also=learn_mean)
            now = {"Logloss": res["logloss"], "AUC": res["auc"]}
        ev = model.evals_result_
        ev["learn"]["Logloss"].append(learn)
        for name, value in now.items():
            ev["validation"].setdefault(name, []).append(value)
        score = -now["Logloss"] if metric == "Logloss" else now[metric]
        if state["best"] is None or score > state["best"]:
            state["best"], state["since"] = score, 0
            model.best_iteration_ = len(ev["validation"]["AUC"]) - 1
            model.best_score_ = {"validation": now}
            if use_best_model:
                with torch.no_grad():
                    if snapshot is None:
                        snapshot = [torch.empty_like(p) for p in params]
                    torch._foreach_copy_(snapshot, params)
                stale = False
        else:
            state["since"] += 1
        return early_stopping_rounds is not None and state["since"] >= early_stopping_rounds

    stop, gstep = False, 0
    since_total = torch.zeros((), device=dev, dtype=torch.float64)
    since_rows = 0
    for _ in range(epochs):
        order = torch.randperm(R, generator=gen).to(dev) if shuffle else None
        total = torch.zeros((), device=dev, dtype=torch.float64)
        for s in range(0, R, batch_size):
            e = min(R, s + batch_size)
            loss = step(slice(s, e) if order is None else order[s:e])
            row_loss = loss * (e - s) if tr.reduction == "mean" else loss
            total += row_loss
            stale = True
            gstep += 1
            if eval_every is not None:
                since_total += row_loss
                since_rows += e - s
                if gstep % eval_every == 0:
                    stop = evaluate_now(since_total / since_rows)
                    since_total.zero_()
                    since_rows = 0
                    if stop:
                        break
        if stop:
            break       # the epoch was cut short: no mean for it
        mean = total / R
        if eval_every is None:
            stop = evaluate_now(mean)
            means.append(model.evals_result_["learn"]["Logloss"][-1])
            if stop:
                break
        else:
            means.append(float(mean.item()))
    if after_steps is not None:
        after_steps()
    if use_best_model and snapshot is not None and stale:
        before = [p._version for p in params]
        with torch.no_grad():
            for p, s in zip(params, snapshot):
                p.copy_(s)
        for p, v in zip(params, before):     # the caches of forward_logits key on the version counters
            if p._version == v:
                torch.autograd.graph.increment_version(p)
    return means


class DeepFM(nn.Module):
    """deepctr-torch-style DeepFM over F sparse fields (binary task).

    Parameter names follow deepctr-torch's module tree (embedding_dict.C{i}, linear_model.
    embedding_dict.C{i}, dnn.linears.{j}, dnn_linear, out.bias) so its checkpoints map 1:1.
    forward(X [R, F] int64) -> prob [R, 1] (as deepctr's BaseModel.forward)."""

    def __init__(self, field_vocab_sizes, embed_dim=16, dnn_hidden_units=(256, 128), init_std=1e-4, seed=1024,
                 device="cpu"):
        super().__init__()
        if embed_dim != 16:
            raise ValueError("the fused kernel is specialised for embed_dim=16 (config 3)")
        torch.manual_seed(seed)
        self.field_names = [f"C{i + 1}" for i in range(len(field_vocab_sizes))]
        self.embed_dim = embed_dim
        self.embedding_dict = nn.ModuleDict(
            {n: nn.Embedding(v, embed_dim) for n, v in zip(self.field_names, field_vocab_sizes)})
        self.linear_model = nn.Module()
        self.linear_model.embedding_dict = nn.ModuleDict(
            {n: nn.Embedding(v, 1) for n, v in zip(self.field_names, field_vocab_sizes)})
        dims = [len(field_vocab_sizes) * embed_dim] + list(dnn_hidden_units)
        self.dnn = nn.Module()
        self.dnn.linears = nn.ModuleList([nn.Linear(dims[i], dims[i + 1]) for i in range(len(dims) - 1)])
        self.dnn_linear = nn.Linear(dims[-1], 1, bias=False)
        self.out = nn.Module()
        self.out.bias = nn.Parameter(torch.zeros((1,)))
        for emb in list(self.embedding_dict.values()) + list(self.linear_model.embedding_dict.values()):
            nn.init.normal_(emb.weight, mean=0, std=init_std)
        for name, t in self.dnn.linears.named_parameters():
            if "weight" in name:
                nn.init.normal_(t, mean=0, std=init_std)
        self.to(device)

    @torch.no_grad()
    def forward(self, X):
        _, prob = self.forward_logits(X)
        return prob.unsqueeze(1)

    def _bias_value(self) -> float:
        """out.bias as a host float, read once per parameter version (no sync per forward)."""
        b = self.out.bias
        c = self.__dict__.get("_bias_cache")
        if c is None or c[0] is not b or c[1] != b._version:
            c = self.__dict__["_bias_cache"] = (b, b._version, float(b.item()))
        return c[2]

    def _param_lists(self):
        """(embedding weights, linear weights, DNN weights, DNN biases, output weight), read through
        the submodules' parameter dicts from a submodule list built once: nn.Module attribute
        lookups for the 80 tensors cost more host time per call than the fused kernel itself.
        A parameter replaced on a submodule is still seen; replacing a submodule is not supported."""
        mods = self.__dict__.get("_mod_lists")
        if mods is None:
            mods = self.__dict__["_mod_lists"] = (
                [self.embedding_dict[n] for n in self.field_names],
                [self.linear_model.embedding_dict[n] for n in self.field_names],
                list(self.dnn.linears), self.dnn_linear)
        emb, lin, dnn, out = mods
        return ([m._parameters["weight"] for m in emb], [m._parameters["weight"] for m in lin],
                [m._parameters["weight"] for m in dnn], [m._parameters["bias"] for m in dnn],
                out._parameters["weight"])

    @torch.no_grad()
    def forward_logits(self, X):
        emb, lin, ws, bs, wo = self._param_lists()
        return ops.deepfm_forward(X, emb, lin, self._bias_value(), ws, bs, wo,
                                  cache=self.__dict__.setdefault("_fused_cache", {}))

    def predict_proba(self, X) -> np.ndarray:
        """CatBoost-compatible: probability of class 1 (RecommendationRanker.predict_proba :148-149)."""
        if not torch.is_tensor(X):
            X = torch.as_tensor(np.asarray(X), dtype=torch.int64)
        dev = next(self.parameters()).device
        return self.forward_logits(X.to(dev))[1].cpu().numpy()

    def make_trainer(self, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, reduction="mean", max_grad_norm=None):
        """A DeepFMTrainer over this model's parameters (Logloss; SparseAdam semantics on the tables,
        Adam on the dense parameters). Raises NotImplementedError for shapes the training kernels do
        not cover (embed_dim 16, dnn_hidden_units (256, 128), 1 <= F <= 64)."""
        return DeepFMTrainer(self, lr, betas, eps, reduction, max_grad_norm)

    def _rows_on_device(self, X, y):
        dev = next(self.parameters()).device
        X = torch.as_tensor(np.asarray(X) if not torch.is_tensor(X) else X).to(dev, torch.int64)
        y = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).to(dev, torch.float32).reshape(-1)
        if X.dim() != 2 or y.numel() != X.shape[0]:
            raise ValueError(f"need X [R, F] and y [R] (got {tuple(X.shape)} and {y.numel()} labels)")
        return X, y

    @torch.no_grad()
    def _evaluate_on_device(self, X, y, batch_size, group=None, top=10):
        """forward_logits over X in batches into one [R] buffer, then one ops.binary_eval (and, with
        group [R] int32, one ops.group_eval: the pair is returned): nothing is read back here
        (forward_logits itself re-reads out.bias, 4 bytes, once after the weights changed)."""
        R = X.shape[0]
        logits = torch.empty(R, device=X.device, dtype=torch.float32)
        for s in range(0, R, batch_size):
            logits[s:s + batch_size].copy_(self.forward_logits(X[s:s + batch_size])[0])
        be = ops.binary_eval(logits, y)
        return be if group is None else (be, ops.group_eval(logits, y, group, top=top))

    def evaluate(self, X, y, batch_size=65536, group_id=None, top=10):
        """{"Logloss", "AUC"} of the model on X [R, F] / y [R] in {0, 1} (tensors or array-likes): the
        fused inference kernel over batches of batch_size (the last short batch included) and one
        device-side evaluation (ops.binary_eval: exact tie-aware ROC-AUC, mean Logloss), one host
        read. AUC is NaN when y holds a single class. With group_id [R] (integers in [0, 2^31), the
        reference's per-customer group id; the rows of a group anywhere) the dict gains "NDCG" (the
        mean tie-averaged NDCG@top over the groups with a positive) and "QueryAUC" (the mean AUC
        over the groups with both classes) from ops.group_eval, still one host read; NaN when no
        group qualifies."""
        X, y = self._rows_on_device(X, y)
        return _evaluate_result(self._evaluate_on_device, (X, y), y, int(batch_size), group_id, top)

    def fit(self, X, y, batch_size, epochs=1, shuffle=True, seed=0, eval_set=None, eval_metric="AUC",
            early_stopping_rounds=None, use_best_model=None, eval_every=None, eval_group_id=None, **trainer_kw):
        """Train on X [R, F] int64 / y [R] in {0, 1} (the slot of RecommendationRanker.train :114-137)
        for `epochs` passes in batches of batch_size (the last short batch included; row order
        shuffled per epoch from `seed`). Returns the completed epochs' mean row losses (one host read
        per epoch). trainer_kw: make_trainer's arguments.

        eval_set=(X_val, y_val) adds the reference's validation (CatBoost's eval_set / eval_metric /
        early_stopping_rounds / use_best_model, :98-108, :123-135): the validation rows are moved to
        the device once and evaluated (as evaluate does) after every epoch, or after every
        eval_every-th training step instead when eval_every is given. eval_metric "AUC" (larger is
        better) or "Logloss" (smaller is better) picks the best evaluation: only a strictly better
        one replaces it. early_stopping_rounds=k stops after k consecutive evaluations without an
        improvement. use_best_model (default True with an eval_set) leaves the model with the
        parameters of the best evaluation: they are copied into a device snapshot at every
        improvement (allocated once, overwritten in place, on the stream) and copied back into the
        same Parameter objects at the end, so the trainer and the inference caches see them. The
        snapshot doubles the model's footprint (2.5 GB more at configuration 3: 39 fields of 10^6
        rows); the optimizer moments are not snapshotted. One host read per evaluation (the metrics,
        with the epoch's mean loss in the same copy) besides forward_logits' 4-byte refresh of
        out.bias; none per step. Records evals_result_ = {"learn": {"Logloss": [...]}, "validation":
        {"Logloss": [...], "AUC": [...]}} (learn: the mean training loss since the previous
        evaluation), best_iteration_ (0-based index of the best evaluation) and best_score_ =
        {"validation": {"Logloss", "AUC"}} at it. ValueError before the first step for an unknown
        eval_metric, validation labels outside {0, 1}, or a single class with eval_metric "AUC".

        eval_group_id [validation rows] (integers in [0, 2^31): the reference's per-customer group id
        of its ranker rows) adds the per-query metrics of evaluate(group_id=...): every evaluation also
        records "NDCG" and "QueryAUC" under evals_result_["validation"] and best_score_["validation"]
        (the binary block, the group block and the learn mean in one copy: still one host read per
        evaluation), and eval_metric may be "NDCG" (NDCG@10), "NDCG:top=K" or "QueryAUC" (larger is
        better). Without it nothing changes. ValueError before the first step for a per-group
        eval_metric without eval_group_id, a malformed or out-of-range ":top=K", a length other than
        the validation rows', an id outside [0, 2^31), "NDCG" with no group that holds a positive or
        "QueryAUC" with no group that holds both classes (one more host read up front)."""
        use_best_model = _fit_args(eval_set, eval_metric, early_stopping_rounds, use_best_model, eval_every,
                                   eval_group_id)
        validate = None
        if eval_set is not None:
            Xv, yv = self._rows_on_device(*eval_set)
            _fit_eval_labels(yv, eval_metric)
            gv = None if eval_group_id is None else _fit_eval_groups(yv, eval_group_id, eval_metric)
            top = _parse_eval_metric(eval_metric)[1]
            validate = lambda: self._evaluate_on_device(Xv, yv, 65536, gv, top)   # noqa: E731
        tr = self.make_trainer(**trainer_kw)
        X, y = self._rows_on_device(X, y)
        return _fit_loop(self, tr, lambda sel: tr.step(X[sel], y[sel]), X.shape[0], X.device, batch_size, epochs,
                         shuffle, seed, validate, eval_metric, early_stopping_rounds, use_best_model, eval_every,
                         after_steps=tr.check_ids)


class DeepFMTrainer:
    """One-call training steps for a DeepFM on the device (ops.deepfm_train_step): step(X, y) runs the
    forward, the Logloss, the backward, the sparse Adam update of the table rows that occur in X
    (torch.optim.SparseAdam semantics, one step count shared by all tables) and Adam on the dense
    parameters (a torch.optim.AdamW(weight_decay=0) stepped by ops.clip_adamw_step, with
    clip_grad_norm_ over the dense parameters when max_grad_norm is given), without a host
    synchronisation. Embedding L2 regularisation is not applied. The trainer holds no validation
    logic: DeepFM.fit(eval_set=...) evaluates between steps (DeepFM.evaluate), stops early and
    restores the best parameters into the same Parameter objects this trainer updates; the moments
    (state_dict) stay those of the last step taken."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, reduction="mean", max_grad_norm=None):
        hidden = [m.out_features for m in model.dnn.linears]
        why = ops.deepfm_train_supported(len(model.field_names), model.embed_dim, hidden)
        if why:
            raise NotImplementedError(why)
        if reduction not in ("mean", "sum"):
            raise ValueError('reduction must be "mean" or "sum"')
        self.model = model
        self.lr, self.betas, self.eps, self.reduction, self.max_grad_norm = lr, tuple(betas), eps, reduction, max_grad_norm
        emb, lin, ws, bs, wo = model._param_lists()
        self.emb_m = [torch.zeros_like(t) for t in emb]
        self.emb_v = [torch.zeros_like(t) for t in emb]
        self.lin_m = [torch.zeros_like(t) for t in lin]
        self.lin_v = [torch.zeros_like(t) for t in lin]
        self.step_count = 0
        self.dense = [ws[0], bs[0], ws[1], bs[1], wo, model.out.bias]
        self.optimizer = torch.optim.AdamW(self.dense, lr=lr, betas=self.betas, eps=eps, weight_decay=0)
        self._guard = ops.IdRangeGuard("DeepFM training ids")
        self._cache = {}

    @torch.no_grad()
    def step(self, X, y):
        """One step on the batch X [R, F] int64, y [R]; returns the loss (0-d device tensor)."""
        m = self.model
        emb, lin, ws, bs, wo = m._param_lists()
        flag = torch.zeros(1, device=emb[0].device, dtype=torch.int32)
        self.step_count += 1
        res = ops.deepfm_train_step(X, y, emb, lin, self.emb_m, self.emb_v, self.lin_m, self.lin_v, m.out.bias, ws, bs,
                                    wo, self.step_count, self.lr, self.betas, self.eps, self.reduction,
                                    id_flag=flag, cache=self._cache)
        self._guard.watch(flag)
        for p, g in zip(self.dense, res.dense):
            p.grad = g.view(p.shape)
        clip = self.dense if self.max_grad_norm is not None else []
        if ops.clip_adamw_step(self.optimizer, clip, self.max_grad_norm or 0.0) is None:
            if self.max_grad_norm is not None:
                torch.nn.utils.clip_grad_norm_(self.dense, self.max_grad_norm)
            self.optimizer.step()
        for p in self.dense:
            p.grad = None
            torch.autograd.graph.increment_version(p)   # rsx_clip_adamw writes through raw pointers
        return res.loss

    def check_ids(self):
        """Raise IndexError if any batch so far held an id outside its field's vocabulary."""
        self._guard.check()

    def state_dict(self):
        """A snapshot (copies): the shared step count, the tables' moments, the dense optimizer's state."""
        import copy
        sd = {name: [t.clone() for t in getattr(self, name)] for name in ("emb_m", "emb_v", "lin_m", "lin_v")}
        sd["step"] = self.step_count
        sd["dense"] = copy.deepcopy(self.optimizer.state_dict())
        return sd

    def load_state_dict(self, sd):
        self.step_count = int(sd["step"])
        for name in ("emb_m", "emb_v", "lin_m", "lin_v"):
            for dst, src in zip(getattr(self, name), sd[name]):
                dst.copy_(src)
        self.optimizer.load_state_dict(sd["dense"])


class FeatureEngineer:
    """Reference :13-89 (per-candidate tabular features for the CatBoost ranker)."""

    def __init__(self):
        self.cat_features = ["season", "gender", "item_category", "item_material", "item_fit", "time_of_day"]

    def create_features(self, user_meta: Dict, item_meta: Dict, two_tower_score: float, user_vector: np.ndarray,
                        item_vector: np.ndarray) -> Dict:
        inter = user_vector * item_vector
        f = {"two_tower_score": two_tower_score, "vec_prod_mean": float(np.mean(inter)),
             "vec_prod_max": float(np.max(inter)), "vec_prod_std": float(np.std(inter)),
             "season": user_meta.get("season", "unknown"), "gender": user_meta.get("gender", "unknown"),
             "user_avg_price": user_meta.get("avg_price", 0.0),
             "item_category": item_meta.get("category", "unknown"),
             "item_material": item_meta.get("material", "unknown"), "item_fit": item_meta.get("fit", "unknown"),
             "item_price": item_meta.get("price", 0)}
        f["price_diff_ratio"] = ((f["item_price"] - f["user_avg_price"]) / f["user_avg_price"]
                                 if f["user_avg_price"] > 0 else 0.0)
        return f

    def prepare_batch(self, batch_data: List[Dict]):
        import pandas as pd
        rows = []
        for d in batch_data:
            row = self.create_features(d["user_meta"], d["item_meta"], d["two_tower_score"], d["user_vector"],
                                       d["item_vector"])
            if "label" in d:
                row["target"] = d["label"]
            rows.append(row)
        return pd.DataFrame(rows)


class RecommendationRanker:
    """Reference :95-149: the boosted-tree ranker over the FeatureEngineer columns, with the reference's
    hyper-parameters (1000 trees of depth 6, learning rate 0.05, Logloss, AUC, early_stopping_rounds 50,
    use_best_model). backend "catboost": CatBoostClassifier, as the reference (constructing it needs
    catboost); "native": ObliviousBoostingClassifier (oblivious_gbdt.py: trained and served on the device,
    a model of its own, not CatBoost's trees); "auto": catboost where it imports, so nothing changes where
    the class worked before, else native. loss_function "QuerySoftMax" (backend "native" only; the default
    stays "Logloss") builds the listwise ObliviousBoostingRanker instead: its rows carry the reference's
    per-customer group id (utils/monitor/log_importer.py) as "group_id", it validates on NDCG@10, and
    its scores are raw scores that order the candidates of a query, not probabilities. one_hot_max_size
    (default None: every categorical column one-hot, at most 255 values each) goes to the native model: a
    categorical column with more known values is encoded by ordered target statistics
    (oblivious_gbdt.py); backend "catboost" ignores it (CatBoost has its own)."""

    def __init__(self, model_path: str = None, backend: str = "auto", loss_function: str = "Logloss",
                 one_hot_max_size: int = None):
        if backend not in ("auto", "catboost", "native"):
            raise ValueError(f'backend must be "auto", "catboost" or "native" (got {backend!r})')
        if loss_function not in ("Logloss", "QuerySoftMax"):
            raise ValueError(f'loss_function must be "Logloss" or "QuerySoftMax" (got {loss_function!r})')
        if loss_function == "QuerySoftMax" and backend != "native":
            raise ValueError('loss_function "QuerySoftMax" needs backend="native"')
        if backend == "auto":
            try:
                import catboost  # noqa: F401
                backend = "catboost"
            except ImportError:
                backend = "native"
        self.backend, self.loss_function = backend, loss_function
        self.engineer = FeatureEngineer()
        if backend == "catboost":
            from catboost import CatBoostClassifier
            self.model = CatBoostClassifier(iterations=1000, learning_rate=0.05, depth=6, loss_function="Logloss",
                                            eval_metric="AUC", verbose=100, early_stopping_rounds=50,
                                            cat_features=self.engineer.cat_features, random_seed=42)
        elif loss_function == "QuerySoftMax":
            from .oblivious_gbdt import ObliviousBoostingRanker
            self.model = ObliviousBoostingRanker(iterations=1000, learning_rate=0.05, depth=6, early_stopping_rounds=50,
                                                 cat_features=self.engineer.cat_features,
                                                 one_hot_max_size=one_hot_max_size)
        else:
            from .oblivious_gbdt import ObliviousBoostingClassifier
            self.model = ObliviousBoostingClassifier(iterations=1000, learning_rate=0.05, depth=6,
                                                     early_stopping_rounds=50,
                                                     cat_features=self.engineer.cat_features,
                                                     one_hot_max_size=one_hot_max_size)
        self.is_fitted = False
        if model_path:
            self.load_model(model_path)

    def train(self, train_data: List[Dict], val_data: List[Dict] = None):
        """Reference :114-137: train_data / val_data are FeatureEngineer.prepare_batch rows with a "label"
        (1 = bought). With val_data the model is validated on it (AUC), stops early and keeps its best
        iteration. With loss_function "QuerySoftMax" every row also carries its "group_id" (an integer >= 0;
        ValueError when one is missing) and the validation metric is NDCG@10."""
        df = self.engineer.prepare_batch(train_data)
        X, y = df.drop(columns=["target"]), df["target"]
        eval_set = None
        if val_data:
            dv = self.engineer.prepare_batch(val_data)
            eval_set = (dv.drop(columns=["target"]), dv["target"])
        if self.loss_function == "QuerySoftMax":
            groups = [_row_group_ids(rows, name) for rows, name in ((train_data, "train_data"), (val_data, "val_data"))]
            self.model.fit(X, y.to_numpy(), groups[0],
                           eval_set=None if eval_set is None else (eval_set[0], eval_set[1].to_numpy()),
                           eval_group_id=groups[1], eval_metric="NDCG:top=10",
                           use_best_model=True if eval_set is not None else None)
        elif self.backend == "catboost":
            self.model.fit(X, y, eval_set=eval_set, use_best_model=True)
        else:
            self.model.fit(X, y.to_numpy(), eval_set=None if eval_set is None else (eval_set[0], eval_set[1].to_numpy()),
                           eval_metric="AUC", use_best_model=True if eval_set is not None else None)
        self.is_fitted = True

    # the FeatureEngineer categorical columns train_rows builds, in the model's order: column -> (whose meta, its key)
    _ROW_CATS = (("season", "user", "season"), ("gender", "user", "gender"), ("item_category", "item", "category"),
                 ("item_material", "item", "material"), ("item_fit", "item", "fit"))

    @torch.no_grad()
    def train_rows(self, rows, item_vectors, user_vectors, item_metadata, user_meta=None, val_rows=None):
        """train without the host rows: rows / val_rows are RankerRows (utils/monitor/log_importer.py:
        HMLogImporter.load_rows, ReRankingSystem.training_rows): row_user, row_item int32 [R] into
        user_vectors [C, d] and item_vectors [N, d], y, group_id and the retrieval score or None, all on the
        device. Backend "native" only (TypeError otherwise). The numeric columns are ops.pair_tabular's (the
        arithmetic of the serving path, ops.rerank_tabular: columns 1..6 of a pair have the same bits in both;
        with score None the two-tower score is the pair's dot product), in the order ops.RERANK_TABULAR_COLUMNS.
        The categorical columns season, gender, item_category, item_material, item_fit are gathered from
        per-user and per-item code tables whose vocabularies are built once from the metadata dicts
        (item_metadata: {item row: dict}, user_meta: C dicts, default {}; a missing key reads "unknown"), in
        the order of first occurrence over the tables. No per-row Python: the host loops run over the N items
        and the C users. The model is fitted through fit((numeric, codes), y[, group_id]) and then carries the
        FeatureEngineer column names and these vocabularies, so ReRankingSystem.rerank_batch /
        recommend_batch serve it and save_model / load_model round-trip it. With val_rows the model validates
        as train does (AUC, or NDCG@10 for QuerySoftMax), stops early and keeps its best iteration. A column
        with more than 255 values raises ValueError unless the ranker was built with one_hot_max_size: then the
        columns with more values than that are target-statistic columns of the fit."""
        if self.backend != "native":
            raise TypeError(f'train_rows needs backend="native" (this ranker\'s is {self.backend!r})')
        dev = rows.row_user.device
        n, C = item_vectors.shape[0], user_vectors.shape[0]
        user_meta = [{}] * C if user_meta is None else list(user_meta)
        if len(user_meta) != C:
            raise ValueError(f"user_meta holds {len(user_meta)} dicts for {C} user vectors")
        metas = {"item": [item_metadata.get(i, {}) for i in range(n)], "user": user_meta}
        price = torch.tensor([float(m.get("price", 0)) for m in metas["item"]], dtype=torch.float32, device=dev)
        avg = torch.tensor([float(m.get("avg_price", 0.0)) for m in metas["user"]], dtype=torch.float32, device=dev)
        vocabs, tables = [], []
        for name, side, key in self._ROW_CATS:
            vocab = {}
            codes = np.fromiter((vocab.setdefault(m.get(key, "unknown"), len(vocab) + 1) for m in metas[side]), np.int64,
                                len(metas[side]))
            if len(vocab) > 255 and self.model.one_hot_max_size is None:      # else fit decides: a TS column
                raise ValueError(f"categorical column {name!r} has {len(vocab)} distinct values: at most 255 are supported")
            vocabs.append(vocab)
            tables.append((side, torch.from_numpy(codes).to(dev)))

        def columns(r):
            feats = ops.pair_tabular(r.row_user, r.row_item, r.score, user_vectors, item_vectors, price, avg)
            idx = {"user": r.row_user.long(), "item": r.row_item.long()}
            return feats.t(), torch.stack([t.index_select(0, idx[side]) for side, t in tables], dim=1)

        X = columns(rows)
        have_val = val_rows is not None and len(val_rows) > 0
        eval_set = (columns(val_rows), val_rows.y) if have_val else None
        if self.loss_function == "QuerySoftMax":
            self.model.fit(X, rows.y, rows.group_id, eval_set=eval_set,
                           eval_group_id=val_rows.group_id if have_val else None, eval_metric="NDCG:top=10",
                           use_best_model=True if have_val else None)
        else:
            self.model.fit(X, rows.y, eval_set=eval_set, eval_metric="AUC", use_best_model=True if have_val else None)
        names = (list(ops.RERANK_TABULAR_COLUMNS), [name for name, _, _ in self._ROW_CATS])
        self.model._fitted_names, self.model.feature_names_, self.model.vocab_ = names, names[0] + names[1], vocabs
        self.is_fitted = True

    def save_model(self, path: str):
        self.model.save_model(path)

    def load_model(self, path: str):
        self.model.load_model(path)
        self.is_fitted = True

    def get_feature_importance(self, *args, **kwargs):
        """The model's get_feature_importance: the native model's (oblivious_gbdt.py: "PredictionValuesChange",
        "ShapValues" or "LossFunctionChange") or CatBoost's own."""
        return self.model.get_feature_importance(*args, **kwargs)

    @property
    def feature_importances_(self):
        return self.model.feature_importances_

    def predict_proba(self, X) -> np.ndarray:
        if self.loss_function == "QuerySoftMax":
            raise TypeError("a QuerySoftMax ranker scores, it has no probabilities: use predict")
        return self.model.predict_proba(X)[:, 1]

    def predict(self, X) -> np.ndarray:
        """The scores that order the rows X (a host array): the raw scores of a QuerySoftMax ranker, else the
        probabilities of class 1."""
        if self.loss_function == "QuerySoftMax":
            return self.model.predict(X).cpu().numpy()
        return self.predict_proba(X)


def _row_group_ids(rows, name):
    """The "group_id" of every row of train_data / val_data as an int64 tensor (None for no rows)."""
    if not rows:
        return None
    missing = sum(1 for d in rows if "group_id" not in d)
    if missing:
        raise ValueError(f'{name}: {missing} of {len(rows)} rows carry no "group_id" (loss_function "QuerySoftMax" '
                         "ranks within groups)")
    return torch.tensor([int(d["group_id"]) for d in rows], dtype=torch.int64)


_HASH_ITEM, _HASH_USER, _HASH_FIELD = 0x9E3779B1, 0x85EBCA77, 0xC2B2AE35


def hashed_cross_features(user_bucket: torch.Tensor, cand_ids: torch.Tensor, vocab_sizes) -> torch.Tensor:
    """Sparse DeepFM rerank ids for (user, candidate) pairs ("39 sparse ids
    per (user, item) derived by hashing (user_bucket, item_id) pairs"): field f of pair (q, j) is
    mix(item * A + bucket[q] * B + f * C) % vocab_f with mix(h) = (h ^ (h >> 29)) & 0x7FFFFFFF.
    user_bucket [Q] int64, cand_ids [Q, K] int64 -> [Q, K, F] int64."""
    F = len(vocab_sizes)
    dev = cand_ids.device
    fld = torch.arange(F, device=dev, dtype=torch.int64).view(1, 1, F)
    h = cand_ids.unsqueeze(-1) * _HASH_ITEM + user_bucket.view(-1, 1, 1) * _HASH_USER + fld * _HASH_FIELD
    voc = torch.as_tensor(list(vocab_sizes), dtype=torch.int64, device=dev).view(1, 1, F)
    return ((h ^ (h >> 29)) & 0x7FFFFFFF) % voc


class ReRankingSystem:
    """Reference :155-237: retrieval (user_vec @ item_vectors.T, top-k) then rerank.

    ranker: a DeepFM (rerank features = `rerank_features(user_vec, candidate_ids)` -> [k, F]
    int64 ids, e.g. hashed (user bucket, item) crosses) or a RecommendationRanker (CatBoost
    on FeatureEngineer rows, as the reference)."""

    def __init__(self, user_tower, item_tower, ranker, item_db_metadata: Dict[int, Dict],
                 item_db_vectors: torch.Tensor, rerank_features=None):
        self.user_tower = user_tower
        self.item_tower = item_tower
        self.ranker = ranker
        self.item_metadata = item_db_metadata
        self.item_vectors = item_db_vectors
        self.rerank_features = rerank_features
        self.device = item_db_vectors.device

    def recommend(self, user_vector: torch.Tensor, user_meta_raw: Dict = None, top_k_retrieval: int = 100,
                  final_k: int = 10):
        uv = user_vector.reshape(1, -1).to(self.device, torch.float32)
        top_scores, top_idx = ops.retrieve_topk(uv, self.item_vectors, top_k_retrieval)
        idx = top_idx[0]
        if isinstance(self.ranker, DeepFM):
            feats = self.rerank_features(uv, idx)
            probs = self.ranker.predict_proba(feats)
        else:
            rows = [{"user_meta": user_meta_raw or {}, "item_meta": self.item_metadata.get(int(i), {}),
                     "two_tower_score": float(s), "user_vector": uv[0].cpu().numpy(),
                     "item_vector": self.item_vectors[int(i)].cpu().numpy()}
                    for s, i in zip(top_scores[0].tolist(), idx.tolist())]
            frame = self.ranker.engineer.prepare_batch(rows)
            listwise = getattr(self.ranker, "loss_function", "Logloss") == "QuerySoftMax"
            probs = self.ranker.predict(frame) if listwise else self.ranker.predict_proba(frame)
        order = np.argsort(probs)[::-1][:final_k]
        idx_cpu = idx.cpu().numpy()
        sc_cpu = top_scores[0].cpu().numpy()
        return [{"product_id": int(idx_cpu[o]), "two_tower_score": float(sc_cpu[o]), "final_score": float(probs[o])}
                for o in order]

    def rerank_batch(self, cand_ids: torch.Tensor, cand_scores: torch.Tensor, user_buckets: torch.Tensor = None,
                     final_k: int = 10, features=None, user_vectors: torch.Tensor = None, user_meta=None):
        """The rerank half of recommend for a batch of queries, on the device. Returns (product ids,
        two-tower scores, final scores), each [Q, final_k].

        DeepFM ranker: candidates [Q, K] (global item ids) -> rerank ids (features(cand_ids,
        user_buckets) -> [Q, K, F]; default the hashed (user bucket, item) crosses of
        hashed_cross_features) -> DeepFM probabilities -> the final_k most probable per query
        (torch.topk: probability desc).

        Native RecommendationRanker (backend "native", trained on FeatureEngineer rows): user_vectors
        [Q, d] and user_meta (a list of Q dicts as recommend's user_meta_raw; default {}) ->
        ops.rerank_tabular (the numeric FeatureEngineer columns of every candidate from the item
        vectors and the per-item / per-user price tensors) -> ops.gbdt_bin with the model's borders,
        the categorical codes gathered from per-item code tables built once from item_db_metadata (a
        target-statistic column of the model: the bins of its table, an unseen value as code 0) ->
        ops.gbdt_predict -> torch.topk. user_buckets and features are not used. A QuerySoftMax ranker orders by
        its raw score and returns it as the final score (no sigmoid)."""
        if _is_native_ranker(self.ranker):
            if user_vectors is None:
                raise ValueError("rerank_batch with the native tree ranker needs user_vectors [Q, d]")
            return self._rerank_tabular(cand_ids, cand_scores, user_vectors, user_meta, final_k)
        if not isinstance(self.ranker, DeepFM):
            raise TypeError("rerank_batch needs a DeepFM or a native RecommendationRanker (the CatBoost path is "
                            "per-user, recommend)")
        Q, K = cand_ids.shape
        if features is not None:
            feats = features(cand_ids, user_buckets)
        else:
            voc = self.__dict__.get("_vocab")
            if voc is None:
                voc = self.__dict__["_vocab"] = [self.ranker.embedding_dict[n].num_embeddings
                                                 for n in self.ranker.field_names]
            feats = hashed_cross_features(user_buckets, cand_ids, voc)
        _, prob = self.ranker.forward_logits(feats.reshape(Q * K, -1))
        top_p, top_j = torch.topk(prob.view(Q, K), final_k, dim=1)
        return torch.gather(cand_ids, 1, top_j), torch.gather(cand_scores, 1, top_j), top_p

    @torch.no_grad()
    def explain_batch(self, cand_ids: torch.Tensor, cand_scores: torch.Tensor, user_vectors: torch.Tensor, user_meta=None):
        """Why the native tree ranker scores the candidates [Q, K] as it does: (SHAP values float64 [Q, K, F + 1] on
        the device, the F column names followed by "expected_value"). The columns are the model's feature_names_,
        the last entry the expected value, and a candidate's F + 1 entries sum to the raw score rerank_batch
        ranks it by (the logit of its probability for a Logloss model). The bins are the very ones rerank_batch
        scores; arguments as rerank_batch's native path."""
        if not _is_native_ranker(self.ranker):
            raise TypeError("explain_batch needs a native RecommendationRanker")
        Q, K = cand_ids.shape
        clf = self.ranker.model
        phi = clf._shap_of_bins(self._tabular_bins(cand_ids, cand_scores, user_vectors, user_meta))
        return phi.view(Q, K, -1), list(clf.feature_names_) + ["expected_value"]

    def recommend_batch(self, user_vectors: torch.Tensor, user_buckets: torch.Tensor = None,
                        top_k_retrieval: int = 100, final_k: int = 10, user_meta=None):
        """recommend (reference :170-237) for a batch of users with a DeepFM or a native
        RecommendationRanker, entirely on the device: exact top-k retrieval of user_vectors [Q, D]
        against the item vectors (rsx_retrieve_topk), then rerank_batch. user_buckets [Q] int64
        (DeepFM; default: q % 1000); user_meta: Q dicts (native ranker). Returns (product ids,
        two-tower scores, final scores), each [Q, final_k]."""
        uv = user_vectors.to(self.device, torch.float32)
        Q = uv.shape[0]
        if _is_native_ranker(self.ranker):
            sc, idx = ops.retrieve_topk(uv, self.item_vectors, top_k_retrieval)
            return self.rerank_batch(idx, sc, None, final_k, user_vectors=uv, user_meta=user_meta)
        if user_buckets is None:
            user_buckets = torch.arange(Q, device=self.device, dtype=torch.int64) % 1000
        sc, idx = ops.retrieve_topk(uv, self.item_vectors, top_k_retrieval)
        return self.rerank_batch(idx, sc, user_buckets, final_k)

    @torch.no_grad()
    def training_rows(self, user_vectors: torch.Tensor, truth_off: torch.Tensor, truth: torch.Tensor,
                      top_k_retrieval: int = 100):
        """The rows the reranker will see, as a RankerRows for RecommendationRanker.train_rows: the
        top_k_retrieval <= N retrieved candidates of every user vector [Q, d] (ops.retrieve_topk, as
        recommend_batch) with their retrieval scores, group = query, row_user = query, and y = 1 where the
        candidate is in the query's truth set (the CSR of ops.first_hit: truth_off int64 [Q + 1], truth int32
        ascending and distinct per query), labelled by rsx_pair_tabular's y_out. Everything stays on the
        device; nothing is read back."""
        from ..utils.monitor.log_importer import RankerRows
        uv = user_vectors.to(self.device, torch.float32)
        Q, n = uv.shape[0], self.item_vectors.shape[0]
        k = int(top_k_retrieval)
        if not 1 <= k <= n:
            raise ValueError(f"top_k_retrieval must be in [1, {n}] (got {top_k_retrieval})")
        sc, idx = ops.retrieve_topk(uv, self.item_vectors, k)
        query = torch.arange(Q, device=self.device, dtype=torch.int32).repeat_interleave(k)
        row_item = idx.reshape(-1).to(torch.int32)
        zeros = torch.zeros(max(n, Q), device=self.device, dtype=torch.float32)      # the labels need no prices
        _, y = ops.pair_tabular(query, row_item, None, uv, self.item_vectors, zeros[:n], zeros[:Q], truth_off, truth)
        return RankerRows(query, row_item, y, query.clone(), sc.reshape(-1).to(torch.float32).contiguous())


    # the FeatureEngineer columns the meta dicts feed: column -> (whose meta, its key)
    _TABULAR_CATS = {"season": ("user", "season"), "gender": ("user", "gender"),
                     "item_category": ("item", "category"), "item_material": ("item", "material"),
                     "item_fit": ("item", "fit")}

    def _tabular_tables(self, clf):
        """Per-item tensors of the native rerank path, built once per fitted model from item_db_metadata
        (item i = row i of the item vectors): price fp32 [N] and, per categorical item column of the model,
        its codes uint8 [N] under the model's vocabulary; for a target-statistic column the item's bin, its code
        looked up in the model's byte table (ts_bins_), so serving either kind is one one-byte gather."""
        cached = self.__dict__.get("_tabular")
        if cached is not None and cached["model"] is clf.model_:
            return cached
        n = self.item_vectors.shape[0]
        metas = [self.item_metadata.get(i, {}) for i in range(n)]
        nums, cats = clf._fitted_names
        unknown = [c for c in nums if c not in ops.RERANK_TABULAR_COLUMNS]
        if unknown or not clf.vocab_ and cats:
            raise ValueError(f"the native ranker was not fitted on FeatureEngineer rows (columns {unknown or cats})")
        codes = {}
        for k, (name, vocab) in enumerate(zip(cats, clf.vocab_)):
            side, key = self._TABULAR_CATS.get(name, (None, None))
            if side == "item" and k in clf.ts_cols_:       # a TS column: the item's bin, through the model's byte table
                host = np.fromiter((vocab.get(m.get(key, "unknown"), 0) for m in metas), np.int64, n)
                codes[name] = clf._ts_bins_of(k, torch.from_numpy(host).to(self.device))
            elif side == "item":
                host = np.fromiter((vocab.get(m.get(key, "unknown"), 0) for m in metas), np.uint8, n)
                codes[name] = torch.from_numpy(host).to(self.device)
        price = torch.tensor([float(m.get("price", 0)) for m in metas], dtype=torch.float32, device=self.device)
        col = {c: i for i, c in enumerate(ops.RERANK_TABULAR_COLUMNS)}
        rows = [col[c] for c in nums]
        cached = self.__dict__["_tabular"] = {
            "model": clf.model_, "price": price, "codes": codes,
            "rows": None if rows == list(range(len(col))) else torch.tensor(rows, device=self.device)}
        return cached

    @torch.no_grad()
    def _tabular_bins(self, cand_ids, cand_scores, user_vectors, user_meta):
        """The bins uint8 [F, Q K] of the candidates under the native ranker's model, in its internal column
        order: what rerank_batch scores and explain_batch explains."""
        clf = self.ranker.model
        if clf.model_ is None:
            raise RuntimeError("the native ranker is not fitted")
        Q, K = cand_ids.shape
        user_meta = [{}] * Q if user_meta is None else list(user_meta)
        if len(user_meta) != Q:
            raise ValueError(f"user_meta holds {len(user_meta)} dicts for {Q} queries")
        tab = self._tabular_tables(clf)
        uv = user_vectors.to(self.device, torch.float32)
        avg = torch.tensor([float(m.get("avg_price", 0.0)) for m in user_meta], dtype=torch.float32, device=self.device)
        feats, ids = ops.rerank_tabular(cand_ids, cand_scores.to(torch.float32), uv, self.item_vectors, tab["price"], avg)
        nums, cats = clf._fitted_names
        bins = torch.empty(len(nums) + len(cats), Q * K, device=self.device, dtype=torch.uint8)
        if nums:
            x = feats if tab["rows"] is None else feats.index_select(0, tab["rows"])
            ops.gbdt_bin(x, clf.borders_, clf.n_borders_, out=bins)
        rows = clf._cat_rows(len(nums), len(cats))      # numeric, then TS, then one-hot columns
        for k, (name, vocab) in enumerate(zip(cats, clf.vocab_)):
            side, key = self._TABULAR_CATS.get(name, (None, None))
            row = bins[rows[k]]
            if side == "item":
                row.copy_(tab["codes"][name].index_select(0, ids))
            elif side == "user" and k in clf.ts_cols_:
                per_user = torch.tensor([vocab.get(m.get(key, "unknown"), 0) for m in user_meta], dtype=torch.int64,
                                        device=self.device)
                row.copy_(clf._ts_bins_of(k, per_user).repeat_interleave(K))
            elif side == "user":
                per_user = torch.tensor([vocab.get(m.get(key, "unknown"), 0) for m in user_meta], dtype=torch.uint8,
                                        device=self.device)
                row.copy_(per_user.repeat_interleave(K))
            else:
                row.zero_()
        return bins

    @torch.no_grad()
    def _rerank_tabular(self, cand_ids, cand_scores, user_vectors, user_meta, final_k):
        clf = self.ranker.model
        Q, K = cand_ids.shape
        bins = self._tabular_bins(cand_ids, cand_scores, user_vectors, user_meta)
        raw = ops.gbdt_predict(bins, clf.model_).view(Q, K)
        prob = raw if clf.loss_function == "QuerySoftMax" else torch.sigmoid(raw)      # a ranker's score is its raw score
        top_p, top_j = torch.topk(prob, final_k, dim=1)
        return torch.gather(cand_ids, 1, top_j), torch.gather(cand_scores, 1, top_j), top_p


def _is_native_ranker(ranker) -> bool:
    return isinstance(ranker, RecommendationRanker) and ranker.backend == "native"


class CrossNet(nn.Module):
    """Reference :239-272: x_{l+1} = x_0 * (x_l @ k_l + b_l) + x_l, k_l [D, 1] (xavier normal),
    b_l [D] (zeros). GPU forward on rsx_crossnet (one wave per row, the row in registers)."""

    def __init__(self, input_dim, num_layers=3):
        super().__init__()
        self.num_layers = num_layers
        self.kernels = nn.ParameterList([nn.Parameter(torch.nn.init.xavier_normal_(torch.empty(input_dim, 1)))
                                         for _ in range(num_layers)])
        self.biases = nn.ParameterList([nn.Parameter(torch.zeros(input_dim)) for _ in range(num_layers)])

    @torch.no_grad()
    def forward(self, x):
        x_out, _ = ops.crossnet(x, list(self.kernels), list(self.biases), want_x=True)
        return x_out


class RankingModel(nn.Module):
    """Reference :274-357 (DCN-V2 re-ranker): x = cat(user, item[, context]); cross =
    CrossNet(x, 3); deep = GELU(LN(Linear(GELU(LN(Linear(x, 256))), 128))); sigmoid(final_head(
    cat(cross, deep))). Inference on the GPU: the cross network fused with the cross half of
    final_head (rsx_crossnet: neither cross_out nor the concatenation is materialised), the deep
    linears on the fp32-MFMA kernel (rsx_linear_fwd) with the LayerNorm+GELU kernel between;
    dropout is inactive (inference)."""

    def __init__(self, user_dim=128, item_dim=128, context_dim=20):
        super().__init__()
        total_input_dim = user_dim + item_dim + context_dim
        self.cross_net = CrossNet(total_input_dim, num_layers=3)
        self.deep_net = nn.Sequential(nn.Linear(total_input_dim, 256), nn.LayerNorm(256), nn.GELU(), nn.Dropout(0.2),
                                      nn.Linear(256, 128), nn.LayerNorm(128), nn.GELU())
        self.final_head = nn.Linear(total_input_dim + 128, 1)

    def _check_width(self, D):
        if self.deep_net[0].in_features != D:
            raise ValueError(f"input width {D} != the model's {self.deep_net[0].in_features} (context given / omitted?)")

    @torch.no_grad()
    def forward(self, user_emb, item_emb, context_emb=None):
        return torch.sigmoid(self.forward_logits(user_emb, item_emb, context_emb)).unsqueeze(1)

    @torch.no_grad()
    def forward_logits(self, user_emb, item_emb, context_emb=None):
        """The pre-sigmoid logits [B] of forward (the inference path: dropout inactive)."""
        parts = [user_emb, item_emb] + ([context_emb] if context_emb is not None else [])
        x = torch.cat(parts, dim=1).float().contiguous()
        D = x.shape[1]
        lin1, ln1, lin2, ln2 = self.deep_net[0], self.deep_net[1], self.deep_net[4], self.deep_net[5]
        self._check_width(D)
        wh = self.final_head.weight.reshape(-1)
        _, head_part = ops.crossnet(x, list(self.cross_net.kernels), list(self.cross_net.biases), w_head=wh[:D])
        h = ops.layer_norm(ops.linear(x, lin1.weight, lin1.bias), ln1.weight, ln1.bias, ln1.eps,
                           act=ops.ACT_GELU_ERF)
        h = ops.layer_norm(ops.linear(h, lin2.weight, lin2.bias), ln2.weight, ln2.bias, ln2.eps,
                           act=ops.ACT_GELU_ERF)
        return head_part + h @ wh[D:] + self.final_head.bias

    def make_trainer(self, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, reduction="mean",
                     max_grad_norm=None, dropout=None, seed=0):
        """A RankingModelTrainer over this model's parameters (Logloss, AdamW). dropout: the rate after
        the first GELU (default: the module's, nn.Dropout(0.2)); seed: of its masks. Raises
        NotImplementedError for widths the training kernels do not cover (ops.dcn_train_supported)."""
        return RankingModelTrainer(self, lr, betas, eps, weight_decay, reduction, max_grad_norm, dropout, seed)

    def _rows_on_device(self, user, item, context, y):
        dev = self.final_head.weight.device
        parts = [torch.as_tensor(t).to(dev, torch.float32) for t in (user, item, context) if t is not None]
        y = torch.as_tensor(np.asarray(y) if not torch.is_tensor(y) else y).to(dev, torch.float32).reshape(-1)
        if any(t.dim() != 2 or t.shape[0] != y.numel() for t in parts):
            raise ValueError(f"need [R, d] feature blocks and y [R] (got {[tuple(t.shape) for t in parts]} and "
                             f"{y.numel()} labels)")
        self._check_width(sum(t.shape[1] for t in parts))
        return parts, y

    @torch.no_grad()
    def _evaluate_on_device(self, parts, y, batch_size, group=None, top=10):
        """forward_logits over the rows in batches into one [R] buffer, then one ops.binary_eval (and,
        with group [R] int32, one ops.group_eval: the pair is returned)."""
        R = y.numel()
        logits = torch.empty(R, device=y.device, dtype=torch.float32)
        ctx = parts[2] if len(parts) > 2 else None
        for s in range(0, R, batch_size):
            e = s + batch_size
            logits[s:e].copy_(self.forward_logits(parts[0][s:e], parts[1][s:e], None if ctx is None else ctx[s:e]))
        be = ops.binary_eval(logits, y)
        return be if group is None else (be, ops.group_eval(logits, y, group, top=top))

    def evaluate(self, user, item, context, y, batch_size=65536, group_id=None, top=10):
        """{"Logloss", "AUC"} of the model on the rows (user [R, du], item [R, di], context [R, dc] or
        None) against y [R] in {0, 1}: the inference path over batches of batch_size and one
        device-side evaluation (ops.binary_eval), one host read. AUC is NaN when y holds one class.
        group_id [R] adds "NDCG" (at top) and "QueryAUC" as DeepFM.evaluate documents."""
        parts, y = self._rows_on_device(user, item, context, y)
        return _evaluate_result(self._evaluate_on_device, (parts, y), y, int(batch_size), group_id, top)

    def fit(self, user, item, context, y, batch_size, epochs=1, shuffle=True, seed=0, eval_set=None,
            eval_metric="AUC", early_stopping_rounds=None, use_best_model=None, eval_every=None, eval_group_id=None,
            **trainer_kw):
        """Train on the rows (user, item, context or None) / y [R] in {0, 1} with exactly the semantics
        documented on DeepFM.fit (one shared loop): batches of batch_size, the row order shuffled per
        epoch from `seed`, the completed epochs' mean row losses returned; eval_set = (user, item,
        context, y) with eval_metric, early_stopping_rounds, use_best_model (the device snapshot
        restored into the same Parameter objects), eval_every and eval_group_id (the per-query "NDCG" /
        "NDCG:top=K" / "QueryAUC"); evals_result_, best_iteration_, best_score_; the same ValueErrors.
        trainer_kw: make_trainer's other arguments (`seed` also seeds the trainer's dropout masks, so
        one seed reproduces a fit)."""
        use_best_model = _fit_args(eval_set, eval_metric, early_stopping_rounds, use_best_model, eval_every,
                                   eval_group_id)
        validate = None
        if eval_set is not None:
            pv, yv = self._rows_on_device(*eval_set)
            _fit_eval_labels(yv, eval_metric)
            gv = None if eval_group_id is None else _fit_eval_groups(yv, eval_group_id, eval_metric)
            top = _parse_eval_metric(eval_metric)[1]
            validate = lambda: self._evaluate_on_device(pv, yv, 65536, gv, top)   # noqa: E731
        tr = self.make_trainer(seed=seed, **trainer_kw)
        parts, y = self._rows_on_device(user, item, context, y)
        ctx = parts[2] if len(parts) > 2 else None

        def step(sel):
            return tr.step(parts[0][sel], parts[1][sel], None if ctx is None else ctx[sel], y[sel])

        return _fit_loop(self, tr, step, y.numel(), y.device, batch_size, epochs, shuffle, seed, validate, eval_metric,
                         early_stopping_rounds, use_best_model, eval_every)

    @torch.no_grad()
    def predict_for_user(self, user_vec, item_vecs, context_vec=None):
        """Reference :327-357: one user (and context) broadcast over N candidate items -> [N]."""
        if user_vec.dim() == 1:
            user_vec = user_vec.unsqueeze(0)
        n = item_vecs.size(0)
        ctx = None
        if context_vec is not None:
            ctx = (context_vec.unsqueeze(0) if context_vec.dim() == 1 else context_vec).expand(n, -1)
        return self.forward(user_vec.expand(n, -1), item_vecs, ctx).squeeze()


class RankingModelTrainer:
    """One-call training steps for a RankingModel on the device (ops.dcn_train_step): step(user, item,
    context, y) runs the forward (dropout after the first GELU active: a counter-hash mask of (seed,
    step count) that the backward regenerates), the Logloss, the backward (the cross network's on
    rsx_crossnet_bwd) and one torch.optim.AdamW over all parameters (the cross kernels and biases,
    both linears, both LayerNorms, final_head), stepped by ops.clip_adamw_step with clip_grad_norm_
    over them when max_grad_norm is given, without a host synchronisation. The gradient of the
    towers' outputs (user / item / context) is not formed. Validation lives in RankingModel.fit."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, reduction="mean",
                 max_grad_norm=None, dropout=None, seed=0):
        d = model.deep_net
        why = ops.dcn_train_supported(d[0].in_features, (d[0].out_features, d[4].out_features))
        if why:
            raise NotImplementedError(why)
        if reduction not in ("mean", "sum"):
            raise ValueError('reduction must be "mean" or "sum"')
        self.p_drop = float(d[3].p if dropout is None else dropout)
        if not 0.0 <= self.p_drop < 1.0:
            raise ValueError(f"dropout must be in [0, 1) (got {self.p_drop})")
        self.model = model
        self.reduction, self.max_grad_norm, self.seed = reduction, max_grad_norm, int(seed)
        self.step_count = 0
        self.params = (list(model.cross_net.kernels) + list(model.cross_net.biases)
                       + [d[0].weight, d[0].bias, d[1].weight, d[1].bias, d[4].weight, d[4].bias, d[5].weight,
                          d[5].bias, model.final_head.weight, model.final_head.bias])
        self.optimizer = torch.optim.AdamW(self.params, lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay)

    def _mask_seed(self):
        """The dropout seed of the current step: a function of (seed, step count) only."""
        return (self.seed + self.step_count * 0x9E3779B97F4A7C15) & 0xFFFFFFFFFFFFFFFF

    @torch.no_grad()
    def step(self, user, item, context, y, return_step=False):
        """One step on the batch (user [B, du], item [B, di], context [B, dc] or None, y [B]); returns
        the loss (0-d device tensor), or the whole ops.DCNStep with return_step."""
        m = self.model
        parts = [t.float() for t in (user, item, context) if t is not None]
        m._check_width(sum(t.shape[1] for t in parts))
        d, L = m.deep_net, len(m.cross_net.kernels)
        self.step_count += 1
        res = ops.dcn_train_step(parts, y, self.params[:L], self.params[L:2 * L], d[0].weight, d[0].bias, d[1].weight,
                                 d[1].bias, d[4].weight, d[4].bias, d[5].weight, d[5].bias, m.final_head.weight,
                                 m.final_head.bias, eps1=d[1].eps, eps2=d[5].eps, p_drop=self.p_drop,
                                 seed=self._mask_seed(), reduction=self.reduction)
        for p, g in zip(self.params, res.grads):
            p.grad = g.view(p.shape)
        clip = self.params if self.max_grad_norm is not None else []
        if ops.clip_adamw_step(self.optimizer, clip, self.max_grad_norm or 0.0) is None:
            if self.max_grad_norm is not None:
                torch.nn.utils.clip_grad_norm_(self.params, self.max_grad_norm)
            self.optimizer.step()
        for p in self.params:
            p.grad = None
            torch.autograd.graph.increment_version(p)   # rsx_clip_adamw writes through raw pointers
        return res if return_step else res.loss

    def state_dict(self):
        """A snapshot (copies): the step count (it seeds the dropout masks) and the optimizer's state."""
        import copy
        return {"step": self.step_count, "seed": self.seed, "optimizer": copy.deepcopy(self.optimizer.state_dict())}

    def load_state_dict(self, sd):
        self.step_count, self.seed = int(sd["step"]), int(sd["seed"])
        self.optimizer.load_state_dict(sd["optimizer"])
