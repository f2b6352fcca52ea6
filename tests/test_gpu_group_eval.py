"""ops.group_eval (rsx_group_eval) on the device against the per-group reference of
tests/group_eval_ref.py: G, the two group counts and every group's gid, P, N, U2 exactly; every
group's DCG within (L_g + 4) 2^-52 relative (L_g = its rows) and the two means within
(Lmax + G + 8) 2^-52 absolute. The bounds are derived, not measured: each tie group's term is formed
by IEEE-exact operations on inputs the reference shares (the table of ops.ndcg_discounts), a
fixed-order sum of n non-negative doubles is within (n - 1) 2^-53 relative of the exact sum, the
division and the mean of G values in [0, 1] add 2^-53 and (G - 1) 2^-53; doubled as margin.
The kernels work on 2048-row tiles of the rows sorted by (group, -score), so the cases put group and
tie-group boundaries inside tiles, on tile edges and across several tiles."""
import functools
import math

import numpy as np
import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import _native as N
from recsys_amd import ops
from tests import group_eval_ref as GREF

pytestmark = pytest.mark.gpu

SEVEN = np.array([-2.5, -1.0, -0.25, 0.0, 0.5, 1.5, 3.0], dtype=np.float32)
EPS = 2.0 ** -52


def _labels(rng, R, rate=0.4):
    return (rng.random(R) < rate).astype(np.float32)


def _random(R, n_groups, seed, rate=0.4, values=None):
    """Random scores (or draws from `values`), random group ids below n_groups: no group is contiguous."""
    rng = np.random.default_rng(seed)
    z = (rng.standard_normal(R) * 3).astype(np.float32) if values is None else values[rng.integers(0, len(values), R)]
    return z, _labels(rng, R, rate), rng.integers(0, n_groups, R)


def _blocks(sizes, seed, values=None, shuffle=True, ids=None):
    """Groups of the given sizes (ids 0, 1, ... or `ids`), the rows shuffled unless told otherwise."""
    rng = np.random.default_rng(seed)
    R = int(sum(sizes))
    g = np.repeat(np.arange(len(sizes)) if ids is None else np.asarray(ids, dtype=np.int64), sizes)
    z = (rng.standard_normal(R) * 3).astype(np.float32) if values is None else values[rng.integers(0, len(values), R)]
    y = _labels(rng, R)
    if shuffle:
        p = rng.permutation(R)
        z, y, g = z[p], y[p], g[p]
    return z, y, g


def _equal_within_groups(seed):
    z, y, g = _blocks([30] * 100, seed)
    return (g % 7).astype(np.float32) * 0.5 - 1.0, y, g


def _signed_zeros(seed):
    rng = np.random.default_rng(seed)
    R = 3000
    return np.where(rng.random(R) < 0.5, 0.0, -0.0).astype(np.float32), _labels(rng, R), rng.integers(0, 40, R)


def _separable(up):
    """Every group: its positives above (up) or below its negatives, all scores distinct."""
    rng = np.random.default_rng(17)
    R = 5000
    g = rng.integers(0, 60, R)
    y = _labels(rng, R)
    y[:60], g[:60] = 1.0, np.arange(60)        # every group holds both classes
    y[60:120], g[60:120] = 0.0, np.arange(60)
    mag = (rng.permutation(R) + 1).astype(np.float32)
    return np.where((y == 1) == up, mag, -mag).astype(np.float32), y, g


def _three_tiles():
    """Sorted rows: group 0 = rows 0..299, group 1 = rows 300..4799 (it crosses the tile edges 2048
    and 4096, seven values: its tie groups of about 640 rows cross them too), group 2 the rest."""
    return _blocks([300, 4500, 200], 23, values=SEVEN)


CASES = {f"random_{R}": (lambda R=R: _random(R, max(1, R // 8), 100 + R), 10) for R in (1, 2, 63, 64, 65)}
CASES.update({
    "singletons": (lambda: _blocks([1] * 300, 1), 10),
    "one_group_4099": (lambda: _blocks([4099], 2), 10),
    "one_group_4099_seven": (lambda: _blocks([4099], 3, values=SEVEN), 10),
    "groups_of_2048": (lambda: _blocks([2048] * 3, 4), 10),
    "two_groups_2047": (lambda: _random(2047, 2, 5), 10),
    "two_groups_2048": (lambda: _random(2048, 2, 6), 10),
    "two_groups_2049": (lambda: _random(2049, 2, 7), 10),
    "three_tiles": (_three_tiles, 10),
    "equal_within_groups": (lambda: _equal_within_groups(8), 10),
    "seven_values": (lambda: _random(5000, 50, 9, values=SEVEN), 10),
    "signed_zeros": (lambda: _signed_zeros(10), 10),
    "separable_up": (lambda: _separable(True), 10),
    "separable_down": (lambda: _separable(False), 10),
    "sparse_ids": (lambda: _blocks([700, 1500, 900], 11, values=SEVEN, ids=[0, 7, 2 ** 31 - 1]), 10),
    "top_1": (lambda: _random(5000, 50, 12, values=SEVEN), 1),
    "top_above_every_group": (lambda: _random(5000, 50, 13), 1000),
    "top_65536": (lambda: _random(5000, 3, 14, values=SEVEN), 65536),
    "three_tiles_top_65536": (_three_tiles, 65536),      # the DCG sums, not only the counts, cross the tile edges
    "groups_of_6": (lambda: _blocks([6] * 1000, 15, values=SEVEN), 10),
    "groups_of_100": (lambda: _blocks([100] * 60, 16), 10),
    "few_positives": (lambda: _random(6000, 600, 18, rate=0.12), 10),
    "no_positive": (lambda: (_random(3000, 40, 19)[0], np.zeros(3000, np.float32), _random(3000, 40, 19)[2]), 10),
    # the sort merge-sorts up to 1,048,576 rows and runs radix passes beyond: the first case (and every
    # case above) is on the first side, the second one on the other
    "groups_of_100_300000": (lambda: _blocks([100] * 3000, 20), 10),
    "groups_of_100_1048700": (lambda: _blocks([100] * 10487, 21), 10),
})


@functools.lru_cache(maxsize=None)
def _case(name):
    make, top = CASES[name]
    z, y, g = make()
    groups = GREF.per_group(z, y, g, top)
    return z, y, g, top, groups, GREF.summary(groups, top)


def _run(gpu, z, y, g, top, **kw):
    return ops.group_eval(torch.from_numpy(z).to(gpu), torch.from_numpy(y).to(gpu), torch.from_numpy(np.asarray(g)).to(gpu),
                          top=top, **kw)


def _check(ev, groups, want, label):
    """The comparison this file is about; returns the two worst figures for the printout."""
    res = ev.result()
    assert (res["groups"], res["ndcg_groups"], res["auc_groups"]) == (want["groups"], want["ndcg_groups"],
                                                                      want["auc_groups"])
    gid, P, Nn, U2, dcg = (t.cpu().tolist() for t in ev.per_group())
    assert gid == [r["gid"] for r in groups]
    assert P == [r["P"] for r in groups] and Nn == [r["N"] for r in groups]
    assert U2 == [r["U2"] for r in groups]
    worst = 0.0
    for r, d in zip(groups, dcg):
        err, bound = abs(d - r["dcg"]), (r["rows"] + 4) * EPS * r["dcg"]
        assert err <= bound, f"group {r['gid']}: dcg {d!r} reference {r['dcg']!r} bound {bound:.2e}"
        if r["dcg"]:
            worst = max(worst, err / r["dcg"])
    bound = (max(r["rows"] for r in groups) + len(groups) + 8) * EPS
    errs = []
    for key in ("ndcg", "query_auc"):
        if math.isnan(want[key]):
            assert math.isnan(res[key])
        else:
            errs.append(abs(res[key] - want[key]))
            assert errs[-1] <= bound, f"{key} {res[key]!r} reference {want[key]!r} bound {bound:.2e}"
    print(f"[{label}] G {len(groups)}: worst relative dcg error {worst:.2e}, mean errors {errs} (bound {bound:.2e})")
    return res


@pytest.mark.parametrize("name", list(CASES))
def test_against_the_reference(gpu, name):
    z, y, g, top, groups, want = _case(name)
    res = _check(_run(gpu, z, y, g, top), groups, want, name)
    if name == "separable_up":
        assert res["query_auc"] == 1.0 and res["auc_groups"] == 60
        assert abs(res["ndcg"] - 1.0) <= (max(r["rows"] for r in groups) + len(groups) + 8) * EPS
    if name == "separable_down":
        assert res["query_auc"] == 0.0 and res["auc_groups"] == 60
    if name in ("equal_within_groups", "signed_zeros"):
        assert res["query_auc"] == 0.5
    if name == "no_positive":
        assert math.isnan(res["ndcg"]) and math.isnan(res["query_auc"]) and res["ndcg_groups"] == res["auc_groups"] == 0
    if name == "singletons":
        assert res["groups"] == 300 and res["auc_groups"] == 0 and res["ndcg"] == 1.0
    if name == "few_positives":
        # groups without a positive / with one class are left out and counted, and enough groups remain
        G = want["groups"]
        assert 2 * want["ndcg_groups"] >= G and 2 * want["auc_groups"] >= G
        assert want["auc_groups"] <= want["ndcg_groups"] < G


def test_max_group_id_gives_identical_outputs(gpu):
    for name, bound in (("seven_values", 49), ("seven_values", 1000), ("sparse_ids", 2 ** 31 - 1), ("random_1", 0)):
        z, y, g, top, groups, want = _case(name)
        a, b = _run(gpu, z, y, g, top), _run(gpu, z, y, g, top, max_group_id=bound)
        assert torch.equal(_summary_bits(a), _summary_bits(b))
        a.result(), b.result()
        for s, t in zip(a.per_group(), b.per_group()):
            assert torch.equal(s, t)
    z, y, g, top, _, _ = _case("seven_values")
    with pytest.raises(ValueError, match="group id"):      # an id above the bound the caller gave
        _run(gpu, z, y, g, top, max_group_id=48).result()


def test_group_id_dtypes(gpu):
    z, y, g, top, groups, want = _case("seven_values")
    for dt in (torch.int32, torch.int64, torch.int16, torch.uint8):
        ev = ops.group_eval(torch.from_numpy(z).to(gpu), torch.from_numpy(y).to(gpu), torch.from_numpy(g).to(dt), top=top)
        _check(ev, groups, want, str(dt))


@pytest.mark.parametrize("what,match", [("nan", "NaN or infinite"), ("inf", "NaN or infinite"),
                                        ("label", "neither 0 nor 1"), ("group", "group id")])
def test_bad_inputs_raise(gpu, what, match):
    z, y, g, top, _, _ = _case("seven_values")
    z, y, g = z.copy(), y.copy(), g.copy()
    if what == "label":
        y[4000] = 2.0
    elif what == "group":
        g[4000] = -1
    else:
        z[4000] = {"nan": np.nan, "inf": np.inf}[what]
    ev = _run(gpu, z, y, g, top)
    with pytest.raises(ValueError, match=match):
        ev.result()


def test_group_id_beyond_int32_raises(gpu):
    z, y, g, top, _, _ = _case("seven_values")
    g = g.copy()
    g[17] = 2 ** 31
    with pytest.raises(ValueError, match="group id"):
        _run(gpu, z, y, g, top).result()


def _summary_bits(ev):
    """The summary's and the flag's bits (the allocation's last 4 bytes are padding)."""
    return torch.cat([ev.summary, ev.flag.to(torch.int64)]).cpu()


def _all_bits(ev):
    ev.result()
    return [_summary_bits(ev)] + [t.cpu() for t in ev.per_group()]


def test_two_calls_give_identical_bits(gpu):
    for name in ("three_tiles", "groups_of_100_300000", "groups_of_100_1048700"):
        z, y, g, top, _, _ = _case(name)
        zt, yt, gt = torch.from_numpy(z).to(gpu), torch.from_numpy(y).to(gpu), torch.from_numpy(g).to(gpu)
        a, b = ops.group_eval(zt, yt, gt, top=top), ops.group_eval(zt, yt, gt, top=top)
        for s, t in zip(_all_bits(a), _all_bits(b)):
            assert torch.equal(s.view(torch.uint8), t.view(torch.uint8))


def test_permuted_rows(gpu):
    for name in ("three_tiles", "seven_values", "groups_of_100"):
        z, y, g, top, groups, want = _case(name)
        p = np.random.default_rng(99).permutation(len(z))
        _check(_run(gpu, z[p], y[p], g[p], top), groups, want, name + " permuted")


def test_outputs_need_no_zeroing(gpu):
    """The native entry on a workspace and output buffers filled with 0xA5 bytes."""
    z, y, g, top, groups, want = _case("three_tiles")
    R = len(z)
    lib = N.lib()
    nws = lib.rsx_group_eval_workspace_bytes(R)
    zt, yt = torch.from_numpy(z).to(gpu), torch.from_numpy(y).to(gpu)
    gt = torch.from_numpy(g).to(gpu, torch.int32)
    D = ops.ndcg_discounts(top, gpu)

    def junk(n, dtype):
        return torch.full((n * torch.empty((), dtype=dtype).element_size(),), 0xA5, device=gpu, dtype=torch.uint8).view(dtype)

    ws, buf, gid, dcg = junk(nws, torch.uint8), junk(6, torch.int64), junk(R, torch.int32), junk(R, torch.float64)
    P, Nn, U2 = junk(R, torch.int64), junk(R, torch.int64), junk(R, torch.int64)
    flag = buf[5:6].view(torch.int32)[:1]
    N.check(lib.rsx_group_eval(N.ptr(zt), N.ptr(yt), N.ptr(gt), R, top, N.ptr(D), -1, N.ptr(ws), nws, N.ptr(buf),
                               N.ptr(gid), N.ptr(P), N.ptr(Nn), N.ptr(U2), N.ptr(dcg), N.ptr(flag), N.stream()),
            "group_eval")
    ev = ops.GroupEval(buf, R, top, (gid, P, Nn, U2, dcg))
    _check(ev, groups, want, "junk-filled buffers")
    ref = _run(gpu, z, y, g, top)
    for s, t in zip(_all_bits(ev), _all_bits(ref)):
        assert torch.equal(s.view(torch.uint8), t.view(torch.uint8))


def test_per_group_needs_result_first(gpu):
    z, y, g, top, _, _ = _case("random_65")
    with pytest.raises(RuntimeError, match="result"):
        _run(gpu, z, y, g, top).per_group()


def test_fetched_with_a_binary_eval_in_one_copy(gpu):
    z, y, g, top, groups, want = _case("seven_values")
    zt, yt = torch.from_numpy(z).to(gpu), torch.from_numpy(y).to(gpu)
    be, ge = ops.binary_eval(zt, yt), _run(gpu, z, y, g, top)
    extra = torch.tensor([0.1, -7.25], device=gpu, dtype=torch.float64)
    b, gr, also = ops._fetch_evals(be, ge, also=extra)
    assert b == ops.binary_eval(zt, yt).result() and gr == _run(gpu, z, y, g, top).result() and also == [0.1, -7.25]
    res, also = _run(gpu, z, y, g, top).result(also=extra)
    assert res == gr and also == [0.1, -7.25]


def test_shape_and_dtype_errors(gpu):
    z4, g4 = torch.zeros(4, device=gpu), torch.zeros(4, device=gpu, dtype=torch.int64)
    with pytest.raises(ValueError, match="labels for"):
        ops.group_eval(z4, torch.zeros(3, device=gpu), g4)
    with pytest.raises(ValueError, match="group ids for"):
        ops.group_eval(z4, z4, g4[:3])
    with pytest.raises(ValueError, match="float32"):
        ops.group_eval(z4.double(), z4, g4)
    with pytest.raises(ValueError, match="integer dtype"):
        ops.group_eval(z4, z4, z4)
    with pytest.raises(ValueError, match="at least one row"):
        ops.group_eval(z4[:0], z4[:0], g4[:0])
    for top in (0, 65537, 2.5):
        with pytest.raises(ValueError, match="top must be"):
            ops.group_eval(z4, z4, g4, top=top)
    with pytest.raises(ValueError, match="max_group_id"):
        ops.group_eval(z4, z4, g4, max_group_id=2 ** 31)
