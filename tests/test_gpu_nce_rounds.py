"""The fused loss forward's round-filling grid (csrc/nce_common.h: fwdg_schedule) on the device.

With 1 or 2 caller slots the forward runs whole-row workgroups on the leading row blocks, as many as
fill whole rounds of slots = 2 x CUs co-resident workgroups, and up to 8 column splits on the rest. The
cases put the row count just above one round so that both regions are small: a universe of 180 items
(D = 180 distinct targets: 6 column tiles, so two of the tail's 8 splits are empty; same-user
exception columns are dense), and the same rows with the targets folded onto 32 and 33 items (one tile,
one tile plus one column), cut to exactly one round of row blocks (no tail) and to one round plus one
row block.

Reference: oracle.user_tower.inbatch_corrected_logq_loss_chunked in float64 (the ungrouped N x N
formula), one evaluation per case shared by the precisions. Tolerances as tests/test_gpu_fullsize.py:
mean loss 1e-4, dU and dW 1e-3 of their scale."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import recsys_amd  # noqa: F401
from recsys_amd import _native, ops, synth
from oracle import user_tower as O

pytestmark = pytest.mark.gpu

ROWS = 128
# 3,520 users of the 180-item universe draw N = 66,074 valid rows (seed 500): 538 above the 65,536 rows
# of one round at 256 CUs, not a multiple of 128, all 180 items drawn
USERS, ITEMS, SEED = 3520, 180, 500
PRECISIONS = ["f16", "bf16x3"]
_CACHE = {}


def _slots(gpu):
    return 2 * torch.cuda.get_device_properties(gpu).multi_processor_count


def _schedule(n, d):
    sched = (ctypes.c_int64 * 7)()
    assert _native.lib().rsx_nce_fwdg_schedule(n, d, 2, 0, sched, None, 0) == 0   # cus 0: this device's
    return dict(zip(("rb1", "ns1", "span1", "ns2", "span2", "nslots", "blocks"), sched))


def _rows(gpu):
    if "rows" not in _CACHE:
        items = synth.make_items(num_items=ITEMS, d=128, seed=0)
        batch = synth.make_batch(items, USERS, seed=SEED)
        valid = ~batch["padding_mask"]
        t = batch["target_ids"][valid]
        uid = torch.arange(USERS).unsqueeze(1).expand(-1, valid.shape[1])[valid]
        U = F.normalize(torch.randn(t.numel(), 128, generator=torch.Generator().manual_seed(SEED)), dim=1)
        _CACHE["rows"] = (items, t, uid, U)
    return _CACHE["rows"]


def _case(gpu, name):
    """(t, uid, U, Wn, lq, reference loss, dU, dW over the item matrix) of a named case, computed once"""
    if name in _CACHE:
        return _CACHE[name]
    items, t, uid, U = _rows(gpu)
    slots = _slots(gpu)
    assert t.numel() > slots * ROWS and t.numel() % ROWS != 0, (t.numel(), slots)
    if name == "fold32":
        t = t % 32 + 1
    elif name == "fold33":
        t = t % 33 + 1
    elif name == "whole_rounds":
        n = slots * ROWS
        t, uid, U = t[:n], uid[:n], U[:n]
    elif name == "one_more_block":
        n = slots * ROWS + 5
        t, uid, U = t[:n], uid[:n], U[:n]
    else:
        assert name == "both_regions"
    Wn = F.normalize(items.pretrained, dim=1)
    lq = items.log_q
    U64 = U.double().to(gpu).requires_grad_()
    W64 = Wn.double().to(gpu).requires_grad_()
    ref = O.inbatch_corrected_logq_loss_chunked(U64, W64, t.to(gpu), uid.to(gpu), lq.double().to(gpu), chunk=2048)
    ref.backward()
    _CACHE[name] = (t, uid, U, Wn, lq, ref.item(), U64.grad.detach(), W64.grad.detach())
    return _CACHE[name]


def _run(gpu, case, precision):
    t, uid, U, Wn, lq = case[:5]
    Ud = U.to(gpu).requires_grad_()
    groups = ops.TargetGroups(t.to(gpu), uid.to(gpu))
    items_d = Wn.to(gpu)[groups.uniq].clone().requires_grad_()
    s, cnt = ops.nce_grouped_sum(Ud, items_d, lq.to(gpu)[groups.uniq], groups, tau=0.1, tag="rounds",
                                 precision=precision)
    loss = s / cnt
    loss.backward()
    return groups, loss.detach(), int(cnt.item()), Ud.grad.detach(), items_d.grad.detach()


def _check(gpu, name, precision):
    case = _case(gpu, name)
    groups, loss, cnt, dU, dW = _run(gpu, case, precision)
    n = case[0].numel()
    ref_loss, gu_ref, gw_ref = case[5], case[6], case[7][groups.uniq]
    err_l = abs(loss.item() - ref_loss)
    err_u = (dU.double() - gu_ref).abs().max().item() / gu_ref.abs().max().item()
    err_w = (dW.double() - gw_ref).abs().max().item() / gw_ref.abs().max().item()
    print(f"[rounds {name} {precision}] N={n} D={groups.n_cols} |dloss|={err_l:.2e} grad_u {err_u:.2e} grad_w {err_w:.2e}")
    assert cnt == n
    assert err_l < 1e-4, (loss.item(), ref_loss)
    assert err_u <= 1e-3 and err_w <= 1e-3, (err_u, err_w)
    return groups


@pytest.mark.parametrize("precision", PRECISIONS)
def test_leading_and_tail_regions(gpu, precision):
    """One round of whole-row workgroups, then 5 row blocks on 8 splits of one tile each, 2 of them empty."""
    groups = _check(gpu, "both_regions", precision)
    n, d, slots = groups.n_rows, groups.n_cols, _slots(gpu)
    assert 100 <= d <= 200
    s = _schedule(n, d)
    assert s["rb1"] == slots and s["ns1"] == 1 and s["ns2"] == 8 and s["nslots"] == 8
    assert s["span2"] == 32 and -(-d // 32) < 8          # one tile per split, fewer tiles than splits


@pytest.mark.parametrize("fold", [32, 33])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_single_tile_problems(gpu, precision, fold):
    """D = 32: one column tile, every tail split but the first is empty; D = 33: one column in the second."""
    groups = _check(gpu, f"fold{fold}", precision)
    assert groups.n_cols == fold
    s = _schedule(groups.n_rows, groups.n_cols)
    assert s["rb1"] == _slots(gpu) and s["ns2"] == 8 and s["span1"] == 32 * (-(-fold // 32)) and s["span2"] == 32


@pytest.mark.parametrize("name", ["whole_rounds", "one_more_block"])
@pytest.mark.parametrize("precision", PRECISIONS)
def test_whole_rounds_only(gpu, precision, name):
    """Row blocks an exact multiple of the slots (no tail region, one slot per row), and one block more."""
    groups = _check(gpu, name, precision)
    slots = _slots(gpu)
    s = _schedule(groups.n_rows, groups.n_cols)
    rbs = -(-groups.n_rows // ROWS)
    if name == "whole_rounds":
        assert rbs == slots and s["rb1"] == rbs and s["nslots"] == 1 and s["blocks"] == rbs
    else:
        assert rbs == slots + 1 and s["rb1"] == slots and s["ns2"] == 8 and s["blocks"] == slots + 8


@pytest.mark.parametrize("precision", PRECISIONS)
def test_two_calls_are_bit_identical(gpu, precision):
    case = _case(gpu, "both_regions")
    _, l0, _, du0, dw0 = _run(gpu, case, precision)
    _, l1, _, du1, dw1 = _run(gpu, case, precision)
    assert torch.equal(l0, l1) and torch.equal(du0, du1) and torch.equal(dw0, dw1)
