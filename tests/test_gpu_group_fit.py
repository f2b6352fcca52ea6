"""The per-query metrics through the models: DeepFM / RankingModel .evaluate(group_id=...) and
.fit(eval_group_id=..., eval_metric="NDCG:top=K" | "QueryAUC") on the device. The models, rows and
the manual-loop pattern are those of test_gpu_deepfm_eval.py and test_gpu_dcn_train.py: the expected
traces come from a manual make_trainer().step loop with evaluate(group_id=...) between the epochs,
the stopping rule applied to that trace."""
import copy
import functools

import numpy as np
import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import ops
from tests import deepfm_train_ref as REF
from tests.test_gpu_dcn_train import _model as _dcn_model
from tests.test_gpu_dcn_train import _teacher_rows
from tests.test_gpu_deepfm_eval import BS, VOCABS, R, _data, _params_of
from tests.test_gpu_deepfm_train import LR, _model, _model_tensors

pytestmark = pytest.mark.gpu

EPOCHS = 8
DCN_R, DCN_BS = 1024, 384


def _groups(n, size, seed):
    """n rows in groups of `size` (the last one shorter), the ids sparse and the rows of a group scattered."""
    ids = (np.arange(n) // size) * 37 + 5
    return torch.from_numpy(ids[np.random.default_rng(seed).permutation(n)])


def _rule(evals, key, rounds):
    """(best index, index of the last evaluation run): a strictly larger evals[i][key] replaces the
    best, training stops after `rounds` consecutive evaluations that do not."""
    best = since = 0
    for i, e in enumerate(evals):
        if i == 0 or e[key] > evals[best][key]:
            best, since = i, 0
        else:
            since += 1
            if since >= rounds:
                return best, i
    return best, len(evals) - 1


def _validation(model):
    v = model.evals_result_["validation"]
    return [dict(zip(v, vals)) for vals in zip(*v.values())]


# ---- DeepFM ------------------------------------------------------------------------------------------
def test_deepfm_evaluate_with_groups(gpu):
    model = _model(REF.make_params(VOCABS, seed=21), gpu)
    x, y, _, _ = _data("same")
    g = _groups(R, 10, 1)
    plain = model.evaluate(x, y, batch_size=BS)
    got = model.evaluate(x, y, batch_size=BS, group_id=g, top=5)
    assert set(plain) == {"Logloss", "AUC"} and set(got) == {"Logloss", "AUC", "NDCG", "QueryAUC"}
    assert got["Logloss"] == plain["Logloss"] and got["AUC"] == plain["AUC"]      # bit for bit
    xg = x.to(gpu)
    logits = torch.cat([model.forward_logits(xg[s:s + BS])[0] for s in range(0, R, BS)])
    res = ops.group_eval(logits, y.to(gpu), g.to(gpu), top=5).result()
    assert (got["NDCG"], got["QueryAUC"]) == (res["ndcg"], res["query_auc"])
    assert res["groups"] == 100 and 0.0 < got["NDCG"] < 1.0 and 0.0 < got["QueryAUC"] < 1.0
    assert model.evaluate(x.numpy(), y.numpy().tolist(), batch_size=BS, group_id=g.tolist(), top=5) == got
    assert model.evaluate(x, y, group_id=g)["NDCG"] == ops.group_eval(logits, y.to(gpu), g.to(gpu)).result()["ndcg"]
    with pytest.raises(ValueError, match="group_id has"):
        model.evaluate(x, y, group_id=g[:-1])


@functools.lru_cache(maxsize=None)
def _deepfm_manual(top):
    """Validation on the training rows with flipped labels (the better the fit, the worse the order in
    every group): per epoch the metrics, the mean loss and a copy of the parameters."""
    gpu = torch.device("cuda:0")
    x, y, xv, yv = _data("flipped")
    g = _groups(R, 10, 2)
    model = _model(REF.make_params(VOCABS, seed=10), gpu)
    tr = model.make_trainer(lr=LR)
    evals, means, params = [], [], []
    for _ in range(EPOCHS):
        total = torch.zeros((), device=gpu, dtype=torch.float64)
        for s in range(0, R, BS):
            xb, yb = x[s:s + BS].to(gpu), y[s:s + BS].to(gpu)
            total += tr.step(xb, yb) * xb.shape[0]
        means.append(float((total / R).item()))
        evals.append(model.evaluate(xv, yv, group_id=g, top=top))
        params.append(_params_of(model))
    return g, evals, means, params


@pytest.mark.parametrize("metric,key,top", [("NDCG:top=5", "NDCG", 5), ("QueryAUC", "QueryAUC", 10)])
def test_deepfm_fit_with_groups(gpu, metric, key, top):
    x, y, xv, yv = _data("flipped")
    g, evals, means, params = _deepfm_manual(top)
    best, last = _rule(evals, key, 2)
    print(f"[{metric}] manual trace: " + ", ".join(f"{e[key]:.4f}" for e in evals) + f"; best {best}, stop after {last}")
    model = _model(REF.make_params(VOCABS, seed=10), gpu)
    got = model.fit(x, y, batch_size=BS, epochs=EPOCHS, shuffle=False, eval_set=(xv, yv), eval_group_id=g,
                    eval_metric=metric, early_stopping_rounds=2, lr=LR)
    assert got == means[:last + 1]
    assert list(model.evals_result_["validation"]) == ["Logloss", "AUC", "NDCG", "QueryAUC"]
    assert _validation(model) == evals[:last + 1]
    assert model.evals_result_["learn"]["Logloss"] == means[:last + 1]
    assert model.best_iteration_ == best and model.best_score_ == {"validation": evals[best]}
    for (n, a), b in zip(_model_tensors(model), params[best]):
        assert torch.equal(a, b), f"{n} is not the parameter after epoch {best + 1}"
    assert model.evaluate(xv, yv, group_id=g, top=top) == evals[best]


def test_deepfm_fit_without_groups_is_unchanged(gpu):
    x, y, xv, yv = _data("fresh")
    model = _model(REF.make_params(VOCABS, seed=10), gpu)
    model.fit(x, y, batch_size=BS, epochs=2, shuffle=False, eval_set=(xv, yv), lr=LR)
    assert list(model.evals_result_["validation"]) == ["Logloss", "AUC"]
    assert list(model.best_score_["validation"]) == ["Logloss", "AUC"]
    assert list(model.evals_result_["learn"]) == ["Logloss"] and len(model.evals_result_["validation"]["AUC"]) == 2
    # an AUC fit with groups records the same Logloss / AUC trace, plus the two group metrics
    grouped = _model(REF.make_params(VOCABS, seed=10), gpu)
    grouped.fit(x, y, batch_size=BS, epochs=2, shuffle=False, eval_set=(xv, yv), eval_group_id=_groups(600, 6, 3), lr=LR)
    for name in ("Logloss", "AUC"):
        assert grouped.evals_result_["validation"][name] == model.evals_result_["validation"][name]
    assert len(grouped.evals_result_["validation"]["NDCG"]) == len(grouped.evals_result_["validation"]["QueryAUC"]) == 2
    assert grouped.best_iteration_ == model.best_iteration_


def test_deepfm_fit_errors_come_before_the_first_step(gpu):
    x, y, _, _ = _data("same")
    g = _groups(R, 10, 4)
    model = _model(REF.make_params(VOCABS, seed=10), gpu)
    before = _params_of(model)

    def fit(**kw):
        kw.setdefault("eval_set", (x, y))
        return model.fit(x, y, batch_size=BS, lr=LR, **kw)

    for metric in ("NDCG", "NDCG:top=5", "QueryAUC"):
        with pytest.raises(ValueError, match="eval_metric"):
            fit(eval_metric=metric)
    with pytest.raises(ValueError, match="eval_metric must be"):
        fit(eval_metric="PFound", eval_group_id=g)
    with pytest.raises(ValueError, match="eval_metric"):
        fit(eval_metric="NDCG:top=ten", eval_group_id=g)
    with pytest.raises(ValueError, match="top must be"):
        fit(eval_metric="NDCG:top=65537", eval_group_id=g)
    with pytest.raises(ValueError, match="eval_group_id has 999 ids for 1000"):
        fit(eval_metric="NDCG", eval_group_id=g[:-1])
    for bad in (-1, 2 ** 31):
        gb = g.clone()
        gb[500] = bad
        with pytest.raises(ValueError, match="group id"):
            fit(eval_metric="NDCG", eval_group_id=gb)
    with pytest.raises(ValueError, match="holds a positive"):
        fit(eval_set=(x, torch.zeros(R)), eval_metric="NDCG", eval_group_id=g)
    with pytest.raises(ValueError, match="holds both classes"):
        fit(eval_metric="QueryAUC", eval_group_id=torch.arange(R))
    with pytest.raises(ValueError, match="needs an eval_set"):
        fit(eval_set=None, eval_group_id=g)
    for a, b in zip(_params_of(model), before):
        assert torch.equal(a, b)
    # groups of one row each are fine for NDCG
    fit(eval_metric="NDCG", eval_group_id=torch.arange(R))
    assert model.evals_result_["validation"]["NDCG"] == [1.0]
    assert np.isnan(model.evals_result_["validation"]["QueryAUC"][0])


# ---- RankingModel ------------------------------------------------------------------------------------
def _dcn_rows(gpu):
    train = _teacher_rows(DCN_R, 90, gpu)
    return train, (train[0], train[1], train[2], 1.0 - train[3]), _groups(DCN_R, 8, 5)


def test_dcn_evaluate_with_groups(gpu):
    train, val, g = _dcn_rows(gpu)
    m = _dcn_model(True, seed=5).to(gpu)
    plain = m.evaluate(*val, batch_size=DCN_BS)
    got = m.evaluate(*val, batch_size=DCN_BS, group_id=g, top=5)
    assert set(plain) == {"Logloss", "AUC"} and set(got) == {"Logloss", "AUC", "NDCG", "QueryAUC"}
    assert got["Logloss"] == plain["Logloss"] and got["AUC"] == plain["AUC"]
    logits = torch.cat([m.forward_logits(*[t[s:s + DCN_BS] for t in val[:3]]) for s in range(0, DCN_R, DCN_BS)])
    res = ops.group_eval(logits, val[3], g, top=5).result()
    assert (got["NDCG"], got["QueryAUC"]) == (res["ndcg"], res["query_auc"]) and res["groups"] == DCN_R // 8


@functools.lru_cache(maxsize=None)
def _dcn_manual(top):
    gpu = torch.device("cuda:0")
    train, val, g = _dcn_rows(gpu)
    m = _dcn_model(True, seed=6).to(gpu)
    tr = m.make_trainer(lr=LR, seed=3)
    evals, means, params = [], [], []
    for _ in range(EPOCHS):
        total = torch.zeros((), device=gpu, dtype=torch.float64)
        for s in range(0, DCN_R, DCN_BS):
            total += tr.step(*[t[s:s + DCN_BS] for t in train]) * train[0][s:s + DCN_BS].shape[0]
        means.append(float((total / DCN_R).item()))
        evals.append(m.evaluate(*val, group_id=g, top=top))
        params.append([p.detach().clone() for p in m.parameters()])
    return evals, means, params


@pytest.mark.parametrize("metric,key,top", [("NDCG:top=5", "NDCG", 5), ("QueryAUC", "QueryAUC", 10)])
def test_dcn_fit_with_groups(gpu, metric, key, top):
    train, val, g = _dcn_rows(gpu)
    evals, means, params = _dcn_manual(top)
    best, last = _rule(evals, key, 2)
    print(f"[{metric}] manual trace: " + ", ".join(f"{e[key]:.4f}" for e in evals) + f"; best {best}, stop after {last}")
    m = _dcn_model(True, seed=6).to(gpu)
    got = m.fit(*train, batch_size=DCN_BS, epochs=EPOCHS, shuffle=False, eval_set=val, eval_group_id=g,
                eval_metric=metric, early_stopping_rounds=2, lr=LR, seed=3)
    assert got == means[:last + 1]
    assert _validation(m) == evals[:last + 1]
    assert m.best_iteration_ == best and m.best_score_ == {"validation": evals[best]}
    for a, b in zip(m.parameters(), params[best]):
        assert torch.equal(a, b)
    assert m.evaluate(*val, group_id=g, top=top) == evals[best]


def test_dcn_fit_errors_and_unchanged_keys(gpu):
    train, val, g = _dcn_rows(gpu)
    m = _dcn_model(True, seed=6).to(gpu)
    before = copy.deepcopy(m.state_dict())
    with pytest.raises(ValueError, match="eval_metric"):
        m.fit(*train, batch_size=DCN_BS, eval_set=val, eval_metric="NDCG:top=5", lr=LR)
    with pytest.raises(ValueError, match="eval_group_id has"):
        m.fit(*train, batch_size=DCN_BS, eval_set=val, eval_metric="QueryAUC", eval_group_id=g[:10], lr=LR)
    with pytest.raises(ValueError, match="holds both classes"):
        m.fit(*train, batch_size=DCN_BS, eval_set=val, eval_metric="QueryAUC", eval_group_id=torch.arange(DCN_R), lr=LR)
    for k, v in m.state_dict().items():
        assert torch.equal(v, before[k]), k
    m.fit(*train, batch_size=DCN_BS, eval_set=val, lr=LR, seed=3)
    assert list(m.evals_result_["validation"]) == ["Logloss", "AUC"] and list(m.best_score_["validation"]) == ["Logloss", "AUC"]
