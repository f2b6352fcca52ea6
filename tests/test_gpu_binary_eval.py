"""ops.binary_eval (rsx_binary_eval) on the device against the integer reference of
tests/binary_eval_ref.py: P, N and U2 exactly, the AUC bit for bit, the Logloss against float64
binary_cross_entropy_with_logits. The kernels work on 2048-row tiles of the sorted rows, so the
cases put tie groups inside tiles, across tile edges and over whole tiles."""
import functools
import math

import numpy as np
import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import ops
from tests import binary_eval_ref as BREF

pytestmark = pytest.mark.gpu

SEVEN = np.array([-2.5, -1.0, -0.25, 0.0, 0.5, 1.5, 3.0], dtype=np.float32)


def _random(R, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(R) * 3).astype(np.float32), (rng.random(R) < 0.4).astype(np.float32)


def _seven(R, seed):
    rng = np.random.default_rng(seed)
    return SEVEN[rng.integers(0, 7, R)], (rng.random(R) < 0.4).astype(np.float32)


def _equal(R, seed):
    rng = np.random.default_rng(seed)
    return np.full(R, -0.3125, dtype=np.float32), (rng.random(R) < 0.4).astype(np.float32)


def _two_values(R, seed):
    """Two tie groups whose boundary moves with the labels' draw: heads and tails in few tiles only."""
    rng = np.random.default_rng(seed)
    return np.where(rng.random(R) < 0.7, 1.25, -7.0).astype(np.float32), (rng.random(R) < 0.5).astype(np.float32)


def _separable(R, up):
    z = (np.arange(R, dtype=np.float32) - R // 2) * 0.5
    y = (np.arange(R) >= R // 3) if up else (np.arange(R) < R // 3)
    perm = np.random.default_rng(R).permutation(R)
    return z[perm], y[perm].astype(np.float32)


def _signed_zeros(R, seed):
    rng = np.random.default_rng(seed)
    return np.where(rng.random(R) < 0.5, 0.0, -0.0).astype(np.float32), (rng.random(R) < 0.4).astype(np.float32)


CASES = {f"random_{R}": (_random, R, 100 + R) for R in (1, 2, 63, 64, 65, 257, 4099, 70001)}
CASES.update({f"seven_{R}": (_seven, R, 200 + R) for R in (1000, 70001)})
CASES.update({f"equal_{R}": (_equal, R, 300 + R) for R in (4099, 70001)})
# the tile size and its neighbours, and whole tiles only (the vector loads' path with no tail tile)
CASES.update({f"two_values_{R}": (_two_values, R, 400 + R) for R in (2047, 2048, 2049, 6144)})
CASES.update({"seven_6144": (_seven, 6144, 206), "separable_up": (_separable, 5000, True),
              "separable_down": (_separable, 5000, False), "signed_zeros": (_signed_zeros, 3000, 500)})
# the sort changes plan above 262,144 rows (merge sort up to it, radix passes beyond)
CASES.update({"random_262144": (_random, 262144, 601), "random_262145": (_random, 262145, 602),
              "seven_262145": (_seven, 262145, 603)})
EXACT_AUC = {"separable_up": 1.0, "separable_down": 0.0, "signed_zeros": 0.5, "equal_4099": 0.5, "equal_70001": 0.5}


def _bits(ev):
    """Every output's bits (the allocation's last 4 bytes are padding)."""
    return torch.cat([ev.counts, ev.loss_sum.view(torch.int64), ev.flag.to(torch.int64)]).cpu()


@functools.lru_cache(maxsize=None)
def _case(name):
    fn, R, arg = CASES[name]
    z, y = fn(R, arg)
    return z, y, BREF.counts(z, y)


@pytest.mark.parametrize("name", list(CASES))
def test_counts_and_auc_are_exact(gpu, name):
    z, y, (P, N, U2) = _case(name)
    ev = ops.binary_eval(torch.from_numpy(z).to(gpu), torch.from_numpy(y).to(gpu))
    assert [int(v) for v in ev.counts.cpu()] == [P, N, U2]
    res = ev.result()
    assert (res["positives"], res["negatives"]) == (P, N)
    if P and N:
        assert res["auc"] == U2 / (2 * P * N)      # the same correctly rounded quotient: bit for bit
        if name in EXACT_AUC:
            assert res["auc"] == EXACT_AUC[name]
    else:
        assert math.isnan(res["auc"])


def test_single_row_and_single_class(gpu):
    for z, y, want in (([0.7], [1], (1, 0)), ([0.7], [0], (0, 1)), ([0.1, -2.0, 0.1, 5.0], [1, 1, 1, 1], (4, 0))):
        res = ops.binary_eval(torch.tensor(z, device=gpu), torch.tensor(y, device=gpu)).result()
        assert math.isnan(res["auc"]) and (res["positives"], res["negatives"]) == want
        assert math.isfinite(res["logloss"])


def test_label_dtypes_and_unaligned_views(gpu):
    """int64 and bool labels; a logit view that starts 4 bytes into its allocation (the scalar loads)."""
    z, y, (P, N, U2) = _case("random_4099")
    zt = torch.from_numpy(z).to(gpu)
    for lab in (torch.from_numpy(y).long(), torch.from_numpy(y).bool()):
        assert [int(v) for v in ops.binary_eval(zt, lab.to(gpu)).counts.cpu()] == [P, N, U2]
    pz = torch.cat([torch.zeros(1), torch.from_numpy(z)]).to(gpu)[1:]
    py = torch.cat([torch.zeros(1), torch.from_numpy(y)]).to(gpu)[1:]
    a, b = ops.binary_eval(pz, py), ops.binary_eval(zt, torch.from_numpy(y).to(gpu))
    assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("R", [5, 4099, 70001])
def test_logloss_against_float64(gpu, R):
    """|difference| <= 8 * 2^-24 * mean max(1, |z|): the row expression is a few operations on a value
    of magnitude at most |z| + log 2, summed in double."""
    rng = np.random.default_rng(R)
    z = (rng.standard_normal(R) * 4).astype(np.float32)
    z[:4] = (30.0, -30.0, 80.0, -80.0)
    y = (rng.random(R) < 0.4).astype(np.float32)
    y[:5] = (1, 1, 0, 0, 1)       # +30 / -80 right, -30 / +80 wrong: both branches of the expression
    zt, yt = torch.from_numpy(z), torch.from_numpy(y)
    ref = float(torch.nn.functional.binary_cross_entropy_with_logits(zt.double(), yt.double()))
    got = ops.binary_eval(zt.to(gpu), yt.to(gpu)).result()["logloss"]
    bound = 8 * 2.0 ** -24 * float(np.maximum(1.0, np.abs(z.astype(np.float64))).mean())
    print(f"R {R}: logloss {got!r} float64 {ref!r} difference {abs(got - ref):.3e} bound {bound:.3e}")
    assert abs(got - ref) <= bound
    assert abs(got - BREF.logloss_sum(z, y) / R) <= bound


def test_two_calls_give_identical_bits(gpu):
    for name in ("random_70001", "seven_70001"):
        z, y, _ = _case(name)
        zt, yt = torch.from_numpy(z).to(gpu), torch.from_numpy(y).to(gpu)
        a, b = ops.binary_eval(zt, yt), ops.binary_eval(zt, yt)
        assert torch.equal(_bits(a), _bits(b))


@pytest.mark.parametrize("what,match", [("nan", "NaN or infinite"), ("inf", "NaN or infinite"),
                                        ("neg_inf", "NaN or infinite"), ("label", "neither 0 nor 1")])
def test_bad_inputs_raise(gpu, what, match):
    z, y, _ = _case("random_4099")
    z, y = z.copy(), y.copy()
    if what == "label":
        y[4000] = 0.5
    else:
        z[4000] = {"nan": np.nan, "inf": np.inf, "neg_inf": -np.inf}[what]
    ev = ops.binary_eval(torch.from_numpy(z).to(gpu), torch.from_numpy(y).to(gpu))
    with pytest.raises(ValueError, match=match):
        ev.result()


def test_shape_and_dtype_errors(gpu):
    with pytest.raises(ValueError, match="labels for"):
        ops.binary_eval(torch.zeros(4, device=gpu), torch.zeros(3, device=gpu))
    with pytest.raises(ValueError, match="float32"):
        ops.binary_eval(torch.zeros(4, device=gpu, dtype=torch.float64), torch.zeros(4, device=gpu))
    with pytest.raises(ValueError, match="at least one row"):
        ops.binary_eval(torch.zeros(0, device=gpu), torch.zeros(0, device=gpu))
