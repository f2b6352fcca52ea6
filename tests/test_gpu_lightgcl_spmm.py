"""rsx_spmm_norm, rsx_lowrank_proj and rsx_lowrank_update (ops.spmm_norm / lowrank_proj /
lowrank_update_) against float64 (tests/lightgcl_ref.py), element by element within the
recursive-summation bounds, and bit for bit between two launches. The graph's own fp32 dinv is exact
input. Shapes sit on the kernels' edges: rows longer than the chunk length by one and by several
chunks, a row count that is no multiple of the rows per workgroup, one tile of the projection +- 1,
several partial slots, and more tiles than slots."""
import functools

import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import ops
from recsys_amd.gnn_model import v1_lightgcl as G
from tests import lightgcl_ref as REF

pytestmark = pytest.mark.gpu

CHUNK = ops.SPMM_CHUNK
TILE = ops.LOWRANK_ROWS_PER_WG


@functools.lru_cache(maxsize=None)
def _graph(name):
    """(NormAdjacency on the CPU, dense float64 A^), built once per graph."""
    if name == "empty":
        adj = G.NormAdjacency(torch.zeros(2, 0, dtype=torch.int64), 1, 0)
    elif name == "one_edge":
        adj = G.NormAdjacency(torch.tensor([[0], [0]]), 1, 1)
    elif name == "isolated":
        adj = G.NormAdjacency(torch.tensor([[0, 2, 4], [1, 1, 3]]), 5, 5)
    elif name == "star":
        adj = G.NormAdjacency(REF.star_edges(3 * CHUNK + 1), 3 * CHUNK + 1, 1)
    elif name == "power_law":
        adj = G.NormAdjacency(REF.power_law_edges(), 3001, 500)
        assert adj.n % ops.SPMM_ROWS_PER_WG != 0 and adj.long_rows.numel() >= 2
    return adj, REF.dense_norm(adj)


def _rand(n, d, seed):
    return torch.randn(n, d, generator=torch.Generator().manual_seed(seed))


def _check(got, want, bound, what):
    err = (got.cpu().double() - want).abs()
    over = err > bound
    assert not bool(over.any()), (f"{what}: {int(over.sum())} elements over their bound, worst "
                                  f"{float((err / bound.clamp(min=1e-300))[over].max()):.3g} x bound")


def _spmm(gpu, name, D, with_r, alpha=1.0, rows=None, ld=None):
    adj, A = _graph(name)
    X = _rand(adj.n, D, 1)
    R = _rand(adj.n, D, 2) if with_r else None
    got = ops.spmm_norm(adj.to(gpu), _strided(X, ld, gpu), R.to(gpu) if with_r else None, alpha=alpha,
                        rows=None if rows is None else rows.to(gpu))
    want, bound = REF.spmm(A, X, R, alpha, rows)
    assert got.shape == want.shape
    _check(got, want, bound, f"spmm {name} D={D}")
    return got


def _strided(X, ld, gpu):
    """X on the device; with ld as the [:, :D] view of an [n, ld] buffer (row stride ld)."""
    if ld is None:
        return X.to(gpu)
    buf = torch.zeros(X.shape[0], ld, device=gpu)
    buf[:, :X.shape[1]] = X.to(gpu)
    view = buf[:, :X.shape[1]]
    assert view.stride(0) == ld and not view.is_contiguous()
    return view


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("name,with_r,alpha", [
    ("empty", True, 0.5), ("empty", False, 1.0), ("one_edge", True, 1.0), ("isolated", False, 1.0),
    ("isolated", True, 1.0 / 3), ("star", False, 1.0), ("star", True, 1.0 / 3), ("power_law", False, 1.0),
    ("power_law", True, 1.0 / 3)])
def test_spmm_norm_against_float64(gpu, name, with_r, alpha, D):
    _spmm(gpu, name, D, with_r, alpha)


@pytest.mark.parametrize("D", [64, 128])
def test_spmm_norm_listed_rows(gpu, D):
    adj, _ = _graph("power_law")
    g = torch.Generator().manual_seed(5)
    subset = torch.randperm(adj.n, generator=g)[:333]
    long_rows = adj.long_rows[:2]
    repeats = torch.cat([subset[:50], subset[:50], long_rows, long_rows, torch.tensor([0, adj.n - 1])])
    full = _spmm(gpu, "power_law", D, True, 1.0 / 3)
    for rows in (subset, repeats, torch.zeros(0, dtype=torch.int64)):
        got = _spmm(gpu, "power_law", D, True, 1.0 / 3, rows=rows)
        assert got.shape == (rows.numel(), D)
        # the listed-rows form sums a long row's chunks in the same order as the full form
        assert torch.equal(got, full[rows.to(gpu)])
    star = _graph("star")[0]
    _spmm(gpu, "star", D, False, 1.0, rows=torch.tensor([star.n - 1, 0, star.n - 1]))


@pytest.mark.parametrize("D", [64, 128])
def test_spmm_norm_strided_input(gpu, D):
    a = _spmm(gpu, "power_law", D, True, 0.25, ld=D + 4)
    b = _spmm(gpu, "power_law", D, True, 0.25)
    assert torch.equal(a, b)


def test_spmm_norm_refuses_aliasing_and_bad_shapes(gpu):
    adj, _ = _graph("isolated")
    adj = adj.to(gpu)
    X = torch.zeros(adj.n, 64, device=gpu)
    with pytest.raises(ValueError):
        ops.spmm_norm(adj, X, out=X)
    with pytest.raises(ValueError):
        ops.spmm_norm(adj, torch.zeros(adj.n, 96, device=gpu))
    with pytest.raises(ValueError):
        ops.spmm_norm(adj, torch.zeros(adj.n + 1, 64, device=gpu))


LOWRANK_N = [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 17]


@pytest.mark.parametrize("D", [64, 128])
@pytest.mark.parametrize("q", [1, 5, 8])
@pytest.mark.parametrize("n", LOWRANK_N)
def test_lowrank_proj_and_update(gpu, n, q, D):
    _lowrank(gpu, n, q, D)


def test_lowrank_more_tiles_than_slots(gpu):
    """Past 512 tiles a workgroup sums several tiles into its slot."""
    _lowrank(gpu, ops.LOWRANK_MAX_SLOTS * TILE + 300, 5, 64)


def _lowrank(gpu, n, q, D):
    X, V = _rand(n, D, 11), _rand(n, q, 12)
    W, Y = _rand(q, D, 13), _rand(n, D, 14)
    P = ops.lowrank_proj(V.to(gpu), X.to(gpu))
    want, bound = REF.proj(V, X)
    assert P.shape == (q, D)
    _check(P, want, bound, f"lowrank_proj n={n} q={q} D={D}")
    assert torch.equal(P, ops.lowrank_proj(V.to(gpu), X.to(gpu)))
    Yd = Y.to(gpu)
    assert ops.lowrank_update_(Yd, V.to(gpu), W.to(gpu)) is Yd
    want, bound = REF.update(Y, V, W)
    _check(Yd, want, bound, f"lowrank_update n={n} q={q} D={D}")
    assert torch.equal(Yd, ops.lowrank_update_(Y.to(gpu), V.to(gpu), W.to(gpu)))


def test_lowrank_proj_of_no_rows_is_zero(gpu):
    P = ops.lowrank_proj(torch.zeros(0, 5, device=gpu), torch.zeros(0, 64, device=gpu))
    assert torch.equal(P, torch.zeros(5, 64, device=gpu))


@pytest.mark.parametrize("name", ["star", "power_law"])
def test_two_launches_are_bit_identical(gpu, name):
    adj, _ = _graph(name)
    adj = adj.to(gpu)
    X, R = _rand(adj.n, 64, 1).to(gpu), _rand(adj.n, 64, 2).to(gpu)
    a = ops.spmm_norm(adj, X, R, alpha=1.0 / 3)
    b = ops.spmm_norm(adj, X, R, alpha=1.0 / 3)
    assert torch.equal(a, b)
    rows = torch.arange(adj.n - 1, -1, -7, device=gpu)
    assert torch.equal(ops.spmm_norm(adj, X, R, rows=rows), ops.spmm_norm(adj, X, R, rows=rows))
