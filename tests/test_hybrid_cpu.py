"""HybridUserTower without a GPU: tests/hybrid_ref.py against the outputs recorded from the reference's
own model (tests/golden/hybrid_b5), the module's PyTorch composition against hybrid_ref, the state_dict
contract, the reference's zeroed GNN user vector, a user without history, and the argument checks of the
new native entry points."""
import ctypes
import functools
import math
import os

import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import _native, ops
from recsys_amd.tower_code import mined_inference as MI
from tests import hybrid_ref as R

UNIT_ATOL = 2e-6   # fp32 accuracy on unit vectors: the recorded outputs are the reference's fp32 CPU run


@functools.lru_cache(maxsize=None)
def _golden():
    return R.load_golden()


@functools.lru_cache(maxsize=None)
def _model():
    return R.build(MI.HybridUserTower)


def _inputs():
    t, _ = _golden()
    return {k[3:]: v for k, v in t.items() if k.startswith("in.")}


@functools.lru_cache(maxsize=None)
def _ref_forward():
    return R.forward(R.f64(_model().state_dict()), _inputs())


def _call(model, inp):
    return model(inp["u_idx"], inp["seq_ids"], inp["seq_deltas"], inp["seq_mask"], inp["u_dense"], inp["u_cat"])


def test_golden_shape_and_recipe():
    t, meta = _golden()
    inp = _inputs()
    assert tuple(inp["seq_ids"].shape) == (5, 7) and inp["seq_mask"].sum(1).tolist() == [7, 1, 3, 7, 5]
    assert {0, 1000, 1001} <= set(inp["seq_deltas"].flatten().tolist())
    assert meta["n_items"] == 41 and meta["n_users"] == 6
    R.check_recipe(_model().state_dict(), meta)


def test_ref_agrees_with_the_reference_outputs():
    t, _ = _golden()
    out, v, ratios = _ref_forward()
    val = R.valid(_inputs()["seq_mask"])
    for name, got, want in (("output", out, t["out.output"]), ("v_seq", v, t["out.v_seq"])):
        err = float((got - want.double())[val].abs().max())
        print(f"hybrid_ref vs recorded {name}: max |diff| at valid positions {err:.3g}")
        assert err <= UNIT_ATOL, name
    for got, want in zip(ratios, t["out.gate_ratios"].tolist()):
        assert abs(got - want) <= 1e-6, (ratios, t["out.gate_ratios"])


def test_module_composition_agrees_with_ref():
    t, _ = _golden()
    with torch.no_grad():
        out, v, ratios = _call(_model(), _inputs())
    ref_out, ref_v, ref_ratios = _ref_forward()
    val = R.valid(_inputs()["seq_mask"])
    assert out.shape == (5, 7, 128) and v.shape == (5, 7, 128) and len(ratios) == 2
    assert float((out.double() - ref_out)[val].abs().max()) <= UNIT_ATOL
    assert float((v.double() - ref_v)[val].abs().max()) <= UNIT_ATOL
    assert max(abs(a - b) for a, b in zip(ratios, ref_ratios)) <= 1e-6
    # the recorded run is the same fp32 arithmetic: the composition reproduces it
    assert float((out - t["out.output"])[val].abs().max()) <= UNIT_ATOL


def test_module_in_training_mode_keeps_gradients():
    m = R.build(MI.HybridUserTower)
    m.train()
    torch.manual_seed(0)
    out, v, ratios = _call(m, _inputs())
    assert out.requires_grad and torch.isfinite(out).all()
    out.square().sum().backward()
    assert m.seq_adapter.content_proj[0].weight.grad is not None
    assert m.fusion_layer.context_gate[2].weight.grad.abs().sum() > 0


def test_state_dict_contract():
    _, meta = _golden()
    m = _model()
    sd = m.state_dict()
    assert list(sd.keys()) == list(meta["parameters"].keys())
    assert [list(v.shape) for v in sd.values()] == [p[0] for p in meta["parameters"].values()]
    gu, gi, ct = R.make_tables(seed=5)
    torch.manual_seed(3)
    other = MI.HybridUserTower(R.N_USERS, R.N_ITEMS, gu, gi, ct)
    gate_out = other.fusion_layer.context_gate[2]
    assert float(gate_out.weight.detach().abs().max()) == 0.0   # the reference's initial gate
    assert float((gate_out.bias.detach() + 5.0).abs().max()) == 0.0
    res = other.load_state_dict(sd, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in other.state_dict().items():
        assert torch.equal(v, sd[k]), k


def test_gnn_user_table_does_not_reach_the_output():
    """Reference :672 replaces the GNN user vector by zeros: gnn_user_emb and gnn_projector are dead."""
    m = R.build(MI.HybridUserTower)
    with torch.no_grad():
        base, _, _ = _call(m, _inputs())
        m.gnn_user_emb.weight.zero_()
        for p in m.gnn_projector.parameters():
            p.mul_(3.0)
        out, _, _ = _call(m, _inputs())
    assert torch.equal(out, base)


def test_user_without_history_gives_finite_rows():
    inp = R.make_inputs(3, 7, (4, 0, 7), seed=2)
    assert inp["seq_mask"][1].sum() == 0
    m = _model()
    with torch.no_grad():
        out, v, ratios = _call(m, inp)
        enc = MI.encode_users(m, **inp)
    assert torch.isfinite(out).all() and torch.isfinite(v).all() and all(r == r for r in ratios)
    ref_out, _, _ = R.forward(R.f64(m.state_dict()), inp)
    assert float((out.double() - ref_out).abs().max()) <= UNIT_ATOL      # every row, the empty user's too
    assert torch.equal(enc, out[torch.arange(3), torch.tensor([3, 0, 6])])


def test_collate_right_pads():
    batch = [{"user_idx": torch.tensor(u), "user_dense": torch.zeros(3), "user_cat": torch.tensor(0),
              "seq_ids": torch.tensor(ids), "seq_deltas": torch.tensor(ids) * 2, "target_ids": torch.tensor(ids) + 1}
             for u, ids in ((0, [5, 6, 7]), (1, [9]))]
    u_idx, u_dense, u_cat, seq_ids, seq_deltas, seq_mask, target_ids, last_target = MI.user_tower_collate_fn(batch)
    assert seq_ids.tolist() == [[5, 6, 7], [9, 0, 0]] and seq_mask.tolist() == [[1, 1, 1], [1, 0, 0]]
    assert seq_deltas.tolist() == [[10, 12, 14], [18, 0, 0]] and last_target.tolist() == [8, 10]
    assert u_idx.tolist() == [0, 1] and u_dense.shape == (2, 3)


def test_temperature_and_feature_importance():
    m = _model()
    t = m.get_current_temperature(1.0)
    assert t.requires_grad   # the temperature stays a function of the learnt logit_scale
    assert abs(float(t.detach()) - 1.0 / min(max(math.exp(float(m.logit_scale.detach())), 1.0), 100.0)) < 1e-7
    assert set(m.get_meta_feature_importance()) == {"Price", "Count", "Recency", "Channel"}


def test_ffn_rejects_unknown_activation():
    with pytest.raises(ValueError):
        ops.ffn(torch.zeros(2, 128), torch.zeros(512, 128), None, torch.zeros(128, 512), None, act="tanh")
    assert ops.EPI_RELU == 3


# ------------------------------------------------------------------------- native argument checks
def _lib():
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built")
    return _native.load()


P = ctypes.c_void_p(64)   # a non-null, 16-byte aligned pointer that is never dereferenced


def _adapter(lib, **kw):
    a = dict(content=P, ldc=128, Nc=41, Dc=128, gnn=P, ldg=64, Ng=41, Dg=64, ids=P, first_row=0, R=8, w=P,
             deltas=None, time_tab=None, merged=P)
    a.update(kw)
    return lib.rsx_hybrid_adapter_fwd(a["content"], a["ldc"], a["Nc"], a["Dc"], a["gnn"], a["ldg"], a["Ng"], a["Dg"],
                                      a["ids"], a["first_row"], a["R"], a["w"], P, P, P, P, P, P, P, 1e-5, 1e-12,
                                      a["deltas"], a["time_tab"], 1.0, a["merged"], None, None, P, None)


def test_adapter_rejects_bad_arguments():
    lib = _lib()
    for kw, msg in (({"Dc": 64}, b"128 wide"), ({"Dg": 128}, b"64 wide"), ({"content": None}, b"null tensor"),
                    ({"gnn": None}, b"null tensor"), ({"w": None}, b"null tensor"),
                    ({"merged": None}, b"no output"), ({"ids": None, "first_row": 40}, b"exceeds the tables"),
                    ({"ldc": 126}, b"leading dimensions")):
        assert _adapter(lib, **kw) == 1, kw
        assert msg in lib.rsx_last_error(), (kw, lib.rsx_last_error())
    rc = lib.rsx_hybrid_adapter_fwd(P, 128, 41, 128, P, 64, 41, 64, P, 0, 8, P, P, P, P, P, P, P, P, 1e-5, 1e-12, None,
                                    None, 1.0, None, None, P, P, None)   # seq_in without deltas
    assert rc == 1 and b"deltas" in lib.rsx_last_error()


def test_seq_gather_rejects_bad_arguments():
    lib = _lib()
    assert lib.rsx_hybrid_seq_gather(P, 40, 64, 1, P, P, 8, P, 1.0, P, P, None) == 1
    assert b"128 wide" in lib.rsx_last_error()
    assert lib.rsx_hybrid_seq_gather(None, 40, 128, 1, P, P, 8, P, 1.0, P, P, None) == 1
    assert b"null tensor" in lib.rsx_last_error()


def _fuse(lib, **kw):
    a = dict(seq_out=P, B=2, L=7, D=128, hidden=64, u=P, out=P, gate=None, ws=None, ws_bytes=0)
    a.update(kw)
    return lib.rsx_hybrid_fuse_fwd(a["seq_out"], a["B"], a["L"], a["D"], None, 0, a["u"], P, P, P, a["hidden"], P, P, P,
                                   P, 1e-5, 1e-12, a["out"], None, a["gate"], a["ws"], a["ws_bytes"], P, None)


def test_fuse_rejects_bad_arguments():
    lib = _lib()
    for kw, msg in (({"D": 64}, b"128 wide"), ({"hidden": 32}, b"64 wide"), ({"L": 65}, b"L must be"),
                    ({"L": 0}, b"L must be"), ({"seq_out": None}, b"null tensor"), ({"u": None}, b"null tensor"),
                    ({"out": None}, b"null tensor"), ({"gate": P}, b"workspace")):
        assert _fuse(lib, **kw) == 1, kw
        assert msg in lib.rsx_last_error(), (kw, lib.rsx_last_error())
    assert lib.rsx_hybrid_fuse_slots(0) == 0 and lib.rsx_hybrid_fuse_slots(65) == 2
    assert lib.rsx_hybrid_fuse_slots(1 << 30) == 256


def test_relu_epilogue_rejects_aux_and_dropout():
    lib = _lib()
    args = lambda aux, p: (P, 128, P, 128, None, 4, 512, 128, 3, aux, 512, p, 0, P, 512)  # noqa: E731
    assert lib.rsx_gemm_x3(*args(P, 0.0), None) == 1 and b"inference only" in lib.rsx_last_error()
    assert lib.rsx_gemm_x3(*args(None, 0.25), None) == 1 and b"inference only" in lib.rsx_last_error()
    assert lib.rsx_gemm_x3_ws(*args(P, 0.0), None, 0, None) == 1 and b"inference only" in lib.rsx_last_error()
    assert lib.rsx_gemm_x3(P, 128, P, 128, None, 4, 512, 128, 4, None, 0, 0.0, 0, P, 512, None) == 1
    assert b"epi must be" in lib.rsx_last_error()


def test_module_rejects_l65_from_the_native_path():
    """L = 65 is outside the kernels (and rsx_hybrid_fuse_fwd says so); the module then takes the
    PyTorch composition instead of failing."""
    inp = R.make_inputs(2, 65, (65, 3), seed=4)
    m = _model()
    assert not m.native_ok(inp["seq_ids"])
    with torch.no_grad():
        out, _, _ = _call(m, inp)
    assert out.shape == (2, 65, 128) and torch.isfinite(out).all()
