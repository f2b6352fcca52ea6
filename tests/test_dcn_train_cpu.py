"""CPU checks of the DCN-V2 training reference (tests/dcn_train_ref.py) and of the argument refusals
of ops.crossnet_bwd / ops.dcn_train_step, which fire before anything touches a device."""
import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import ops
from recsys_amd.temp_model.ranker_skelet import RankingModel
from oracle import ranker as OR
from tests import dcn_train_ref as REF

F64 = torch.float64


def _cross_case(B, D, L, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, D, generator=g, dtype=F64)
    ks = [torch.randn(D, 1, generator=g, dtype=F64) / D ** 0.5 for _ in range(L)]
    bs = [torch.randn(D, generator=g, dtype=F64) * 0.5 for _ in range(L)]
    wh = torch.randn(D, generator=g, dtype=F64) / D ** 0.5
    return x, ks, bs, wh, torch.randn(B, generator=g, dtype=F64), torch.randn(B, D, generator=g, dtype=F64)


@pytest.mark.parametrize("form", ["dhead", "dx_out", "both"])
@pytest.mark.parametrize("D", [4, 12])
@pytest.mark.parametrize("L", [0, 1, 3])
def test_closed_form_cross_backward_equals_autograd(L, D, form):
    x, ks, bs, wh, dhead, dxo = _cross_case(5, D, L, seed=10 * L + D)
    leaves = [t.clone().requires_grad_() for t in [x, wh] + ks + bs]
    xl, head = REF.cross_head(leaves[0], leaves[2:2 + L], leaves[2 + L:], leaves[1])
    use_h, use_x = form != "dx_out", form != "dhead"
    loss = (head * dhead).sum() * use_h + (xl * dxo).sum() * use_x
    auto = torch.autograd.grad(loss, leaves, allow_unused=True)
    dk, db, dwh, dx = REF.crossnet_bwd(x, ks, bs, wh if use_h else None, dhead if use_h else None,
                                       dxo if use_x else None)
    torch.testing.assert_close(dx, auto[0], rtol=1e-12, atol=1e-12)
    if use_h:
        torch.testing.assert_close(dwh, auto[1], rtol=1e-12, atol=1e-12)
    else:
        assert dwh is None
    for l in range(L):
        torch.testing.assert_close(dk[l], auto[2 + l].reshape(-1), rtol=1e-12, atol=1e-12)
        torch.testing.assert_close(db[l], auto[2 + L + l], rtol=1e-12, atol=1e-12)


def _randomised(model, seed):
    g = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for b in model.cross_net.biases:
            b.copy_(torch.randn(b.shape, generator=g) * 0.1)
        for i in (1, 5):
            model.deep_net[i].weight.copy_(1.0 + 0.2 * torch.randn(model.deep_net[i].weight.shape, generator=g))
            model.deep_net[i].bias.copy_(0.1 * torch.randn(model.deep_net[i].bias.shape, generator=g))
    return model


@pytest.mark.parametrize("context", [True, False])
def test_reference_forward_equals_the_oracle(context):
    torch.manual_seed(3)
    model = _randomised(RankingModel(128, 128, 20 if context else 0), 4)
    g = torch.Generator().manual_seed(5)
    user, item = torch.randn(7, 128, generator=g), torch.randn(7, 128, generator=g)
    ctx = torch.randn(7, 20, generator=g) if context else None
    x = torch.cat([user, item] + ([ctx] if context else []), 1)
    logits, _, _ = REF.forward(model.state_dict(), x)
    want = OR.ranking_model_forward(model, user, item, ctx).squeeze(1)
    torch.testing.assert_close(torch.sigmoid(logits), want.detach(), rtol=1e-13, atol=1e-13)
    assert REF.param_names(model.state_dict()) == [n for n, _ in model.named_parameters()]


def _cross_args(D=8, B=3, L=2):
    x = torch.zeros(B, D)
    return x, [torch.zeros(D, 1) for _ in range(L)], [torch.zeros(D) for _ in range(L)], torch.zeros(D), torch.zeros(B)


def test_crossnet_bwd_refuses_bad_arguments_before_any_launch():
    x, ks, bs, wh, dh = _cross_args()
    with pytest.raises(TypeError, match="x must be float32"):
        ops.crossnet_bwd(x.double(), ks, bs, wh, dh)
    with pytest.raises(TypeError, match=r"kernels\[1\] must be float32"):
        ops.crossnet_bwd(x, [ks[0], ks[1].double()], bs, wh, dh)
    with pytest.raises(TypeError, match="dhead must be float32"):
        ops.crossnet_bwd(x, ks, bs, wh, dh.long())
    with pytest.raises(ValueError, match="2 kernels but 1 biases"):
        ops.crossnet_bwd(x, ks, bs[:1], wh, dh)
    with pytest.raises(ValueError, match=r"biases\[0\] has 4 elements"):
        ops.crossnet_bwd(x, ks, [torch.zeros(4), bs[1]], wh, dh)
    with pytest.raises(ValueError, match="x has 12 columns"):
        ops.crossnet_bwd(torch.zeros(3, 12), ks, bs, wh, dh)
    with pytest.raises(ValueError, match="dhead has 2 elements"):
        ops.crossnet_bwd(x, ks, bs, wh, dh[:2])
    with pytest.raises(ValueError, match="dx_out has shape"):
        ops.crossnet_bwd(x, ks, bs, dx_out=torch.zeros(3, 4))
    with pytest.raises(ValueError, match="w_head and dhead go together"):
        ops.crossnet_bwd(x, ks, bs, wh, None, dx_out=torch.zeros(3, 8))
    with pytest.raises(ValueError, match="no upstream gradient"):
        ops.crossnet_bwd(x, ks, bs)
    with pytest.raises(ValueError, match="must be 2-D"):
        ops.crossnet_bwd(torch.zeros(8), ks, bs, wh, dh)
    with pytest.raises(RuntimeError, match=r"biases\[1\] is on meta"):
        ops.crossnet_bwd(x, ks, [bs[0], torch.zeros(8, device="meta")], wh, dh)
    with pytest.raises(RuntimeError, match="need a ROCm GPU tensor"):   # valid arguments, but there is no CPU path
        ops.crossnet_bwd(x, ks, bs, wh, dh)


def _step_args(D=276, B=3, L=3):
    a = dict(x=torch.zeros(B, D), y=torch.zeros(B), kernels=[torch.zeros(D, 1) for _ in range(L)],
             biases=[torch.zeros(D) for _ in range(L)], w1=torch.zeros(256, D), b1=torch.zeros(256),
             ln1_w=torch.ones(256), ln1_b=torch.zeros(256), w2=torch.zeros(128, 256), b2=torch.zeros(128),
             ln2_w=torch.ones(128), ln2_b=torch.zeros(128), w_head=torch.zeros(1, D + 128), head_bias=torch.zeros(1))
    return a


def test_dcn_train_step_refuses_bad_arguments_before_any_launch():
    def call(exc, match, **over):
        a = _step_args()
        a.update(over)
        with pytest.raises(exc, match=match):
            ops.dcn_train_step(**a)

    call(TypeError, "x must be float32", x=torch.zeros(3, 276, dtype=F64))
    call(TypeError, "w1 must be float32", w1=torch.zeros(256, 276, dtype=torch.bfloat16))
    call(TypeError, "ln2_b must be float32", ln2_b=torch.zeros(128, dtype=F64))
    call(TypeError, "y must be a tensor", y=[0.0, 1.0, 0.0])
    call(ValueError, r"w1 has shape \(256, 256\)", w1=torch.zeros(256, 256))
    call(ValueError, r"w2 has shape", w2=torch.zeros(128, 128))
    call(ValueError, "w_head has 276 elements", w_head=torch.zeros(1, 276))
    call(ValueError, "2 labels for 3 rows", y=torch.zeros(2))
    call(ValueError, r"kernels\[2\] has 256 elements", kernels=[torch.zeros(276, 1)] * 2 + [torch.zeros(256, 1)])
    call(ValueError, "3 kernels but 2 biases", biases=[torch.zeros(276)] * 2)
    call(ValueError, "reduction must be", reduction="none")
    call(ValueError, "p_drop must be in", p_drop=1.0)
    call(ValueError, "at least one row", x=torch.zeros(0, 276), y=torch.zeros(0))
    call(ValueError, r"x\[1\] has 2 rows", x=[torch.zeros(3, 128), torch.zeros(2, 148)])
    call(RuntimeError, "b1 is on meta", b1=torch.zeros(256, device="meta"))
    call(RuntimeError, "y is on meta", y=torch.zeros(3, device="meta"))
    call(RuntimeError, "need a ROCm GPU tensor")
    d = 274   # not a multiple of 4: no kernel covers it
    a = _step_args(D=d)
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        ops.dcn_train_step(**a)


def test_trainer_refuses_widths_and_settings_on_the_cpu():
    with pytest.raises(NotImplementedError, match="multiple of 4"):
        RankingModel(128, 128, 18).make_trainer()
    with pytest.raises(ValueError, match="reduction must be"):
        RankingModel().make_trainer(reduction="none")
    m = RankingModel()
    tr = m.make_trainer(dropout=0.0, seed=3)
    assert tr.p_drop == 0.0 and m.make_trainer().p_drop == 0.2
    assert [id(p) for p in tr.params] == [id(p) for p in m.parameters()]
    with pytest.raises(ValueError, match="input width 256"):
        tr.step(torch.zeros(2, 128), torch.zeros(2, 128), None, torch.zeros(2))
    with pytest.raises(ValueError, match="input width 256"):
        m.evaluate(torch.zeros(2, 128), torch.zeros(2, 128), None, torch.zeros(2))
    with pytest.raises(ValueError, match="eval_metric must be"):
        m.fit(torch.zeros(2, 128), torch.zeros(2, 128), torch.zeros(2, 20), torch.zeros(2), 2, eval_metric="F1")
    with pytest.raises(ValueError, match="need an eval_set"):
        m.fit(torch.zeros(2, 128), torch.zeros(2, 128), torch.zeros(2, 20), torch.zeros(2), 2, early_stopping_rounds=2)
