"""CPU checks of gnn_model/distill_mag_to_cos_l2.py: MagnitudeEncoder's module surface and initialisation
against the reference's module tree, its CPU forward against float64, tests/distill_ref's hand-derived
backward against float64 autograd (plain, masked, the |Z| < eps rows, a pre-activation at exactly 0),
edge_batches, the width limit and the argument checks of the raw ops."""
import math

import pytest
import torch
import torch.nn as nn

import recsys_amd  # noqa: F401
from recsys_amd import ops
from recsys_amd.gnn_model import distill_mag_to_cos_l2 as DM
from recsys_amd.gnn_model import v1_lightgcl as G
from tests import distill_ref as REF

F64 = torch.float64


def _params(seed=0):
    torch.manual_seed(seed)
    m = DM.MagnitudeEncoder()
    return m, [p.detach().clone() for p in (m.encoder[0].weight, m.encoder[0].bias, m.encoder[3].weight,
                                             m.encoder[3].bias, m.logit_scale)]


def _batch(B, seed, nu=301, ni=200):
    U, I = REF.make_tables(nu, ni, 7)
    g = torch.Generator().manual_seed(seed)
    users, items = torch.randint(0, nu, (B,), generator=g), torch.randint(0, ni, (B,), generator=g)
    items[0] = 0     # the all-zero padding row
    if B > 4:
        users[1], items[2] = users[3], items[4]
    return REF.stack(U, I, users, items)


def test_module_surface_and_initialisation():
    for seed in (0, 3):
        torch.manual_seed(seed)
        m = DM.MagnitudeEncoder()
        torch.manual_seed(seed)
        enc = nn.Sequential(nn.Linear(64, 128), nn.LeakyReLU(0.2), nn.Dropout(0.1), nn.Linear(128, 64))
        scale = nn.Parameter(torch.ones([]) * math.log(1 / 0.07))
        sd = m.state_dict()
        assert list(sd) == ["logit_scale", "encoder.0.weight", "encoder.0.bias", "encoder.3.weight", "encoder.3.bias"]
        assert {k: tuple(v.shape) for k, v in sd.items()} == {
            "logit_scale": (), "encoder.0.weight": (128, 64), "encoder.0.bias": (128,),
            "encoder.3.weight": (64, 128), "encoder.3.bias": (64,)}
        for k, v in enc.state_dict().items():
            assert torch.equal(sd["encoder." + k], v), k
        assert torch.equal(sd["logit_scale"], scale.detach())
        assert float(m.logit_scale.detach()) == pytest.approx(math.log(1 / 0.07), rel=1e-7)
        assert m.encoder[1].negative_slope == 0.2 and m.encoder[2].p == 0.1
    wide = DM.MagnitudeEncoder(input_dim=32, output_dim=16, hidden_dim=48)
    assert wide.widths == (32, 48, 16)


def test_cpu_forward_against_float64():
    m, params = _params()
    m.eval()
    X = _batch(37, 1)
    with torch.no_grad():
        y = m(X.float())
    want = REF.forward(X.float().double(), params)[5]
    assert float((y.double() - want).abs().max()) <= 1e-6
    assert float((y.double().norm(dim=1) - 1).abs().max()) <= 1e-6
    # other widths run the same composition
    torch.manual_seed(1)
    wide = DM.MagnitudeEncoder(input_dim=32, output_dim=16, hidden_dim=48).eval()
    out = wide(torch.randn(5, 32))
    assert out.shape == (5, 16) and out.requires_grad


def _autograd(X, params, ks, div=None):
    ps = [p.double().clone().requires_grad_(True) for p in params]
    loss = REF.compose(X, ps, 0.2, ks, 1e-12, div)
    return loss.detach(), torch.autograd.grad(loss, ps)


def _check_backward(X, params, ks, div=None):
    want_loss, want = _autograd(X, params, ks, div)
    got = REF.step(X, params, 0.2, ks, 1e-12, div)
    assert abs(float(got["loss"]) - float(want_loss)) <= 1e-12 * abs(float(want_loss))
    for name, g, w in zip(("w1", "b1", "w2", "b2", "logit_scale"), got["grads"], want):
        assert torch.isfinite(g).all(), name
        assert float((g - w).abs().max()) <= 1e-12 * max(float(w.abs().max()), 1e-300), name
    return got


@pytest.mark.parametrize("masked", [False, True])
def test_reference_backward_against_autograd(masked):
    _, params = _params()
    B = 33
    X = _batch(B, 2)
    ks = REF.keep_scale(1234, 0.1, B) if masked else None
    if masked:
        assert 0.05 < float((ks == 0).double().mean()) < 0.15
    got = _check_backward(X, params, ks)
    assert float(got["grads"][4].abs()) > 0
    _check_backward(X, params, ks, div=B + 1)


def test_reference_backward_degenerate_rows():
    """W2 = 0, b2 = 0: |Z| < eps on every row, the output is 0 and every gradient finite."""
    _, params = _params()
    params[2].zero_()
    params[3].zero_()
    X = _batch(9, 3)
    got = _check_backward(X, params, None)
    assert float(got["rows"].abs().max()) == 0.0
    assert float(got["student"].abs().max()) == 0.0
    assert float(got["grads"][0].abs().max()) == 0.0      # dZ = dY / eps with dY = 0


def test_reference_backward_at_a_zero_preactivation():
    """The padding row is all zero, so its pre-activation is b1: with b1[5] = 0 it is exactly 0 and the
    slope applies there (torch's rule)."""
    _, params = _params()
    params[1][5] = 0.0
    X = _batch(9, 4)
    P = REF.forward(X, params)[0]
    assert float(P[9, 5]) == 0.0       # stacked row B + 0 is item 0
    _check_backward(X, params, None)
    _check_backward(X, params, REF.keep_scale(5, 0.1, 9))


def test_edge_batches():
    g = torch.Generator().manual_seed(0)
    edges = torch.stack([torch.randint(0, 50, (103,), generator=g), torch.randint(0, 40, (103,), generator=g)])

    class NoPerEdgeAccess(G.TrainDataset):
        def __getitem__(self, idx):
            raise AssertionError("edge_batches must not fetch single edges")

        def sample_batch(self, idx, generator=None):
            raise AssertionError("edge_batches must not sample negatives")

    ds = NoPerEdgeAccess(edges, 50, 40)
    it = DM.edge_batches(ds, 25, generator=torch.Generator().manual_seed(5))
    assert len(it) == 5
    epochs = []
    for _ in range(2):
        batches = list(it)
        assert [b[0].numel() for b in batches] == [25, 25, 25, 25, 3]
        assert all(b[2] is None and b[0].dtype == b[1].dtype == torch.int64 for b in batches)
        u, i = torch.cat([b[0] for b in batches]), torch.cat([b[1] for b in batches])
        assert sorted(zip(u.tolist(), i.tolist())) == sorted(zip(edges[0].tolist(), edges[1].tolist()))
        epochs.append((u, i))
    assert not torch.equal(epochs[0][0], epochs[1][0])      # a fresh permutation per epoch
    again = list(DM.edge_batches(ds, 25, generator=torch.Generator().manual_seed(5)))
    assert torch.equal(torch.cat([b[0] for b in again]), epochs[0][0])
    assert torch.equal(torch.cat([b[1] for b in again]), epochs[0][1])
    plain = list(DM.edge_batches(ds, 103, shuffle=False))
    assert len(plain) == 1 and torch.equal(plain[0][0], edges[0]) and torch.equal(plain[0][1], edges[1])


def test_distill_supported_names_the_limit():
    assert ops.distill_supported(64, 128, 64) is None
    for widths in ((128, 128, 64), (64, 256, 64), (64, 128, 128)):
        assert "(64, 128, 64)" in ops.distill_supported(*widths)
    wide = DM.MagnitudeEncoder(input_dim=32, output_dim=16, hidden_dim=48)
    with pytest.raises(NotImplementedError, match=r"\(64, 128, 64\)"):
        wide.make_trainer()
    z = torch.zeros
    with pytest.raises(NotImplementedError, match=r"\(64, 128, 64\)"):
        ops.magnitude_encode(z(3, 64), z(256, 64), z(256), z(64, 256), z(64))


def test_argument_errors_before_any_device_call():
    z = torch.zeros
    good = dict(user_table=z(5, 64), item_table=z(4, 64), users=z(3, dtype=torch.int64),
                items=z(3, dtype=torch.int64), w1=z(128, 64), b1=z(128), w2=z(64, 128), b2=z(64),
                logit_scale=z(()))

    def call(exc, match, **kw):
        with pytest.raises(exc, match=match):
            ops.distill_step(**dict(good, **kw))

    call(TypeError, "user_table must be float32", user_table=z(5, 64, dtype=F64))
    call(TypeError, "w2 must be float32", w2=z(64, 128, dtype=torch.bfloat16))
    call(TypeError, "users must be an integer tensor", users=z(3))
    call(ValueError, "item_table must have 64 columns", item_table=z(4, 32))
    call(ValueError, "user_table must be 2-D", user_table=z(64))
    call(ValueError, "items has 2 elements, expected 3", items=z(2, dtype=torch.int64))
    call(ValueError, "b1 has 64 elements, expected 128", b1=z(64))
    call(ValueError, "logit_scale has 2 elements", logit_scale=z(2))
    call(ValueError, "p_drop must be in", p_drop=1.0)
    call(ValueError, "needs at least one pair", users=z(0, dtype=torch.int64), items=z(0, dtype=torch.int64))
    call(ValueError, "needs exp_avg")
    call(ValueError, "exp_avg has 5 elements", exp_avg=z(5), exp_avg_sq=z(5))
    call(RuntimeError, "item_table is on meta", item_table=z(4, 64, device="meta"))
    call(RuntimeError, "b2 is on meta", b2=z(64, device="meta"))
    call(RuntimeError, "users is on meta", users=z(3, dtype=torch.int64, device="meta"))
    call(RuntimeError, "need a ROCm GPU tensor", update=False)     # valid arguments, but there is no CPU path

    enc = dict(x=z(3, 64), w1=z(128, 64), b1=z(128), w2=z(64, 128), b2=z(64))

    def call_enc(exc, match, **kw):
        with pytest.raises(exc, match=match):
            ops.magnitude_encode(**dict(enc, **kw))

    call_enc(TypeError, "x must be float32", x=z(3, 64, dtype=F64))
    call_enc(ValueError, "x must have 64 columns", x=z(3, 128))
    call_enc(ValueError, "w2 .* does not follow w1", w2=z(64, 64))
    call_enc(ValueError, "eps must be positive", eps=0.0)
    call_enc(RuntimeError, "w1 is on meta", w1=z(128, 64, device="meta"))
    call_enc(RuntimeError, "need a ROCm GPU tensor")


def test_native_argument_errors_without_a_gpu():
    from recsys_amd import _native
    lib = _native.load()
    T = lib.rsx_distill_rows_per_workgroup()
    assert T >= 1
    assert [lib.rsx_distill_slots(b) for b in (0, 1, T, T + 1)] == [0, 1, 1, 2]
    assert lib.rsx_distill_workspace_bytes(T + 1) == 2 * (8 + 4 * ops.DISTILL_PARAMS)
    cap = lib.rsx_distill_slots(1 << 40)
    assert lib.rsx_distill_slots(T * cap + 1) == cap
    p = 16
    assert lib.rsx_magnitude_encode(p, 63, 4, p, p, p, p, 0.2, 1e-12, p, 64, None) == 1
    assert b"leading dimensions" in lib.rsx_last_error()
    assert lib.rsx_magnitude_encode(None, 64, 0, None, None, None, None, 0.2, 1e-12, None, 64, None) == 0
    rc = lib.rsx_distill_grads(p, 64, 5, p, 64, 4, p, p, 3, p, p, p, p, p, 0.2, 0.0, 0, 1e-12, p, 8, None, None,
                               None, p, None)
    assert rc == 1 and b"workspace too small" in lib.rsx_last_error()
    rc = lib.rsx_distill_grads(p, 64, 5, p, 64, 4, p, p, 3, p, p, p, p, p, 0.2, 1.0, 0, 1e-12, p, 1 << 20, None, None,
                               None, p, None)
    assert rc == 1 and b"p_drop" in lib.rsx_last_error()
    rc = lib.rsx_distill_apply(p, 1 << 20, 3, p, p, p, p, p, p, p, None, None, 1, 1e-3, 0.9, 0.999, 1e-8, 0, None)
    assert rc == 1 and b"step counts from 1" in lib.rsx_last_error()
