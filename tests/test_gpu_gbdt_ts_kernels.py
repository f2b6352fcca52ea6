"""rsx_gbdt_ts_keys / rsx_gbdt_ordered_ts (csrc/gbdt_ts.hip) against the integer oracle tests/gbdt_ts_ref.py:
the order, the ordered statistic of every row, the totals and the table, bit for bit, at every tile edge of
the 256-row scan (runs inside a tile, across four tiles, ending exactly on a tile edge), two runs of the same
call, and the range check. The device results and the oracle's are made once per module."""
import numpy as np
import pytest
import torch

from recsys_amd import ops
from tests import gbdt_ts_ref as TS

pytestmark = pytest.mark.gpu

SIZES = (1, 255, 256, 257, 1000)


def _case(name):
    """(codes int64 [Fts, R], y float32 [R], V) of a case."""
    kind, R = name.split(":")
    R = int(R)
    rng = np.random.default_rng(SIZES.index(R) + 70)
    y = (rng.random(R) < 0.35).astype(np.float32)
    if kind == "mixed":          # few long runs and many short ones in one call; one code for all rows; all distinct
        codes = [rng.integers(0, 4, R), rng.integers(0, 2001, R), np.full(R, 2), rng.permutation(R)]
        V = [3, 2000, 3, max(R - 1, 1)]
    elif kind == "edges":        # sorted by code, the runs end exactly at the sorted positions 256 and 512
        codes = [rng.permutation(np.repeat([1, 2, 3], [256, 256, R - 512])), rng.integers(0, 2001, R)]
        V = [3, 2000]
    else:                        # "zeros", "ones": the labels all alike
        codes = [rng.integers(0, 4, R), rng.integers(0, 2001, R)]
        V = [3, 2000]
        y[:] = 1.0 if kind == "ones" else 0.0
    return np.stack(codes).astype(np.int64), y, V


CASES = [f"mixed:{R}" for R in SIZES] + ["edges:1000", "zeros:1000", "ones:1000"]


def _device(gpu, codes, y, V, seed=0, prior=TS.PRIOR):
    c = torch.from_numpy(codes.astype(np.int32)).to(gpu)
    order = ops.gbdt_ts_plan(c, seed)
    return (order,) + ops.gbdt_ordered_ts(c, order, torch.from_numpy(y).to(gpu), V, prior)


@pytest.fixture(scope="module")
def results(gpu):
    out = {}
    for name in CASES:
        codes, y, V = _case(name)
        out[name] = (codes, y, V, _device(gpu, codes, y, V, seed=3))
    ops._GBDT_TS_GUARD.check()
    return out


@pytest.mark.parametrize("name", CASES)
def test_ts_totals_and_table_equal_the_oracle_bit_for_bit(results, name):
    codes, y, V, (order, ts, totals, table) = results[name]
    Fts, R = codes.shape
    assert ts.shape == (Fts, R) and totals.shape == (Fts, max(V) + 1, 2) and table.shape == (Fts, max(V) + 1)
    assert ts.dtype == table.dtype == torch.float32 and totals.dtype == torch.int32
    for j in range(Fts):
        want_ts, want_totals, want_table = TS.ordered_ts(codes[j], y, V[j], seed=3, column=j)
        assert np.array_equal(order[j].cpu().numpy(), TS.sort_key_order(codes[j], TS.hashes(3, j, R))), j
        assert np.array_equal(ts[j].cpu().numpy(), want_ts), j
        assert np.array_equal(totals[j, :V[j] + 1].cpu().numpy(), want_totals), j
        assert np.array_equal(table[j, :V[j] + 1].cpu().numpy(), want_table), j
        assert not totals[j, V[j] + 1:].any() and (table[j, V[j] + 1:] == 0.5).all()     # past V: nobody, p


def test_the_cases_hold_what_they_are_for(results):
    codes, y, _, (_, ts, totals, _) = results["mixed:1000"]
    assert totals[2, 2].tolist() == [1000, int(y.sum())]                  # one run over four tiles
    assert len(np.unique(ts[2].cpu().numpy())) > 100
    assert (ts[3] == 0.5).all()                                           # all codes distinct: exactly p, no label leaks
    by_code = np.sort(results["edges:1000"][0][0])
    assert by_code[255] != by_code[256] and by_code[511] != by_code[512]
    assert (results["zeros:1000"][3][1] <= 0.5).all() and (results["ones:1000"][3][1] >= 0.5).all()


def test_two_calls_give_the_same_bits(gpu, results):
    codes, y, V, first = results["mixed:1000"]
    again = _device(gpu, codes, y, V, seed=3)
    assert all(torch.equal(a, b) for a, b in zip(first, again))


def test_another_prior_and_seed(gpu):
    codes, y, V = _case("edges:1000")
    _, ts, _, table = _device(gpu, codes, y, V, seed=2 ** 40 + 9, prior=(0.3, 2.5))
    for j in range(2):
        want_ts, _, want_table = TS.ordered_ts(codes[j], y, V[j], seed=2 ** 40 + 9, column=j, prior=(0.3, 2.5))
        assert np.array_equal(ts[j].cpu().numpy(), want_ts) and np.array_equal(table[j, :V[j] + 1].cpu().numpy(), want_table)
    ops._GBDT_TS_GUARD.check()


def test_a_code_out_of_range_sets_the_flag_and_gets_p(gpu):
    """Two bad codes (V + 1 and -1): their rows get p and count nowhere, the other rows and the table are those of
    the oracle with the bad rows moved to codes of their own, and the guard raises."""
    codes, y, V = _case("mixed:257")
    codes, V = codes[:2].copy(), V[:2]
    moved = codes.copy()
    codes[0, 5], moved[0, 5] = V[0] + 1, V[0] + 1
    codes[1, 200], moved[1, 200] = -1, V[1] + 1
    ops._GBDT_TS_GUARD.check()
    _, ts, totals, table = _device(gpu, codes, y, V)
    with pytest.raises(IndexError, match="gbdt_ordered_ts"):
        ops._GBDT_TS_GUARD.check()
    assert ts[0, 5] == 0.5 and ts[1, 200] == 0.5
    for j in range(2):
        want_ts, want_totals, want_table = TS.ordered_ts(moved[j], y, V[j] + 1, column=j)
        assert np.array_equal(ts[j].cpu().numpy(), want_ts)
        assert np.array_equal(totals[j, :V[j] + 1].cpu().numpy(), want_totals[:-1])
        assert np.array_equal(table[j, :V[j] + 1].cpu().numpy(), want_table[:-1])


def test_the_wrappers_reject_bad_arguments(gpu):
    c = torch.zeros(2, 10, device=gpu, dtype=torch.int32)
    y = torch.zeros(10, device=gpu)
    order = ops.gbdt_ts_plan(c)
    with pytest.raises(TypeError):
        ops.gbdt_ts_plan(c.long())
    with pytest.raises(ValueError):
        ops.gbdt_ordered_ts(c, order[:1], y, [3, 3])
    with pytest.raises(ValueError, match="known values"):
        ops.gbdt_ordered_ts(c, order, y, [3, ops.GBDT_TS_MAX_CODES + 1])
    with pytest.raises(ValueError, match="prior"):
        ops.gbdt_ordered_ts(c, order, y, [3, 3], prior=(0.5, 0.0))
    with pytest.raises(ValueError):
        ops.gbdt_ordered_ts(c, order, y, [3])
