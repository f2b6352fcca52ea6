"""ops.select_topk_rows (csrc/ensemble.hip, select_topk_k) against np.lexsort: indices and values equal
exactly, in the order (value descending, index ascending), for every row length around the kernel's
steps (one wave's 64, the workgroup's 512, the largest k 2048 and beyond it, a row of several hundred
steps), every k the evaluators use and its limits, and row contents that put ties across the k-th
place. One reference order per (N, content), shared by the k and Q of that case."""
import functools

import numpy as np
import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import ops
from tests import ensemble_ref as REF

pytestmark = pytest.mark.gpu

NS = [1, 7, 255, 256, 257, 2048, 2049, 5000, 70001]
CONTENTS = ["gaussian", "seven_values", "all_equal", "signed_zeros", "low_byte"]
QMAX = 65


@functools.lru_cache(maxsize=None)
def _case(N, content):
    """(S [65, N] float32, the full order of every row by (value descending, index ascending))."""
    rng = np.random.default_rng(1000 * CONTENTS.index(content) + N % 997)
    if content == "gaussian":
        S = rng.standard_normal((QMAX, N)).astype(np.float32)
    elif content == "seven_values":   # about N / 7 ties per value: more ties at the k-th place than places left
        S = rng.choice(np.array([-2.5, -1.0, -0.0, 0.0, 0.5, 0.75, 3.0], dtype=np.float32), size=(QMAX, N))
    elif content == "all_equal":
        S = np.full((QMAX, N), -0.375, dtype=np.float32)
    elif content == "signed_zeros":   # -0.0 and +0.0 tie; a few values on either side
        S = rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1e-3, -1e-3], dtype=np.float32), size=(QMAX, N))
    else:   # the keys agree in their top 24 bits: only the last radix pass separates them
        S = (np.uint32(0x3F800000) | rng.integers(0, 256, size=(QMAX, N)).astype(np.uint32)).view(np.float32)
        S[1::2] *= -1.0
    S = np.ascontiguousarray(S, dtype=np.float32)
    key = REF.score_key(S).astype(np.int64)
    index = np.arange(N)
    order = np.stack([np.lexsort((index, -key[q])) for q in range(QMAX)]).astype(np.int32)
    S.setflags(write=False)
    order.setflags(write=False)
    return S, order


def _ks(N):
    return sorted({k for k in (1, N, min(N, 2048), 1000) if 1 <= k <= min(N, 2048)})


def _check(S_dev, S, order, Q, k):
    idx, val = ops.select_topk_rows(S_dev[:Q], k)
    assert idx.dtype == torch.int32 and idx.shape == (Q, k) and val.shape == (Q, k)
    idx, val = idx.cpu().numpy(), val.cpu().numpy()
    want = order[:Q, :k]
    assert np.array_equal(idx, want), f"indices differ at Q={Q} k={k}"
    want_val = np.take_along_axis(S[:Q], want.astype(np.int64), axis=1)
    assert np.array_equal(val.view(np.uint32), want_val.view(np.uint32)), f"values differ at Q={Q} k={k}"


@pytest.mark.parametrize("content", CONTENTS)
@pytest.mark.parametrize("N", NS)
def test_select_topk_rows_equals_lexsort(gpu, N, content):
    S, order = _case(N, content)
    S_dev = torch.tensor(S).to(gpu)
    for k in _ks(N):
        for Q in (1, 3, QMAX):
            _check(S_dev, S, order, Q, k)


def test_select_topk_rows_reads_strided_rows(gpu):
    S, order = _case(257, "seven_values")
    wide = torch.full((QMAX, 257 + 13), 9.0e9, device=gpu)   # the padding columns would win every place
    wide[:, :257] = torch.tensor(S).to(gpu)
    view = wide[:, :257]
    assert view.stride(0) == 270
    _check(view, S, order, QMAX, 200)


def test_select_topk_rows_is_reproducible(gpu):
    S, _ = _case(5000, "seven_values")
    S_dev = torch.tensor(S).to(gpu)
    a = ops.select_topk_rows(S_dev, 1000)
    b = ops.select_topk_rows(S_dev, 1000)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


def test_select_topk_rows_refuses_k_beyond_its_limits(gpu):
    S = torch.zeros(2, 5000, device=gpu)
    for k in (0, 2049, 5001):
        with pytest.raises(ValueError):
            ops.select_topk_rows(S, k)
