"""CPU checks of the binary evaluation: the integer reference of tests/binary_eval_ref.py against
scikit-learn's roc_auc_score, and the two entry points' argument checks and workspace size (no GPU:
every call below is rejected before a launch, or computes a size on the host)."""
import ctypes
import os

import numpy as np
import pytest

import recsys_amd  # noqa: F401
from recsys_amd import _native
from tests import binary_eval_ref as BREF


def _cases():
    rng = np.random.default_rng(0)
    vals7 = np.array([-2.5, -1.0, -0.25, 0.0, 0.5, 1.5, 3.0], dtype=np.float32)
    zero = np.array([0.0, -0.0] * 20, dtype=np.float32)
    return {
        "seven_values": (vals7[rng.integers(0, 7, 1000)], rng.integers(0, 2, 1000), None),
        "all_equal": (np.full(300, 0.75, dtype=np.float32), rng.integers(0, 2, 300), 0.5),
        "separable_up": (np.arange(200, dtype=np.float32) - 100.0, (np.arange(200) >= 80).astype(np.int64), 1.0),
        "separable_down": (np.arange(200, dtype=np.float32) - 100.0, (np.arange(200) < 80).astype(np.int64), 0.0),
        "signed_zeros": (zero, rng.integers(0, 2, 40), 0.5),
        "signed_zeros_mixed": (np.concatenate([zero, rng.standard_normal(60).astype(np.float32)]),
                               rng.integers(0, 2, 100), None),
    }


@pytest.mark.parametrize("name", list(_cases()))
def test_reference_matches_sklearn(name):
    from sklearn.metrics import roc_auc_score
    z, y, exact = _cases()[name]
    P, N, U2 = BREF.counts(z, y)
    assert P == int(y.sum()) and N == len(y) - P and 0 <= U2 <= 2 * P * N
    got = U2 / (2 * P * N)
    ref = roc_auc_score(y, z.astype(np.float64))
    print(f"[{name}] reference {got!r} sklearn {ref!r} difference {abs(got - ref):.2e}")
    assert abs(got - ref) <= 1e-12
    if exact is not None:
        assert got == exact


def test_reference_single_class_is_nan():
    assert np.isnan(BREF.auc([0.5, 1.0], [1, 1])) and BREF.counts([0.5, 1.0], [1, 1]) == (2, 0, 0)


def _lib():
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built")
    return _native.load()


P16 = ctypes.c_void_p(256)   # a non-null, aligned pointer that is never dereferenced: the calls are rejected first


def test_binary_eval_rejects_bad_arguments_without_a_gpu():
    lib = _lib()
    need = lib.rsx_binary_eval_workspace_bytes(1000)
    assert need > 0

    def call(logit=P16, y=P16, R=1000, ws=P16, ws_bytes=need, counts=P16, loss=P16, flag=P16):
        return lib.rsx_binary_eval(logit, y, R, ws, ws_bytes, counts, loss, flag, None)

    assert call(R=0) == 1 and b"1 <= R < 2^31" in lib.rsx_last_error()
    assert call(R=1 << 31) == 1 and b"1 <= R < 2^31" in lib.rsx_last_error()
    for name in ("logit", "y", "ws", "counts", "loss", "flag"):
        assert call(**{name: None}) == 1 and b"null tensor" in lib.rsx_last_error(), name
    assert call(ws_bytes=need - 1) == 1 and b"workspace too small" in lib.rsx_last_error()
    assert lib.rsx_binary_eval_workspace_bytes(0) == -1 and b"1 <= R < 2^31" in lib.rsx_last_error()
    assert lib.rsx_binary_eval_workspace_bytes(1 << 31) == -1
    with pytest.raises(RuntimeError, match="workspace too small"):
        _native.check(call(ws_bytes=0), "binary_eval")


def test_workspace_bytes_is_non_decreasing():
    """Over the tile size (2048 rows), the powers of two and their neighbours, and the largest R."""
    lib = _lib()
    sweep = set(range(1, 70)) | {(1 << 31) - 1}
    for p in range(6, 31):
        sweep |= {(1 << p) - 1, 1 << p, (1 << p) + 1, 3 << (p - 1)}
    sweep |= {k * 2048 + d for k in (1, 2, 3, 33, 34) for d in (-1, 0, 1)}
    sweep |= {1000, 4099, 65536, 70001, 100000, 1048576, 5000000}
    sizes = [(R, lib.rsx_binary_eval_workspace_bytes(R)) for R in sorted(sweep)]
    for (r0, s0), (r1, s1) in zip(sizes, sizes[1:]):
        assert 0 < s0 <= s1, f"workspace shrinks from R = {r0} ({s0} B) to R = {r1} ({s1} B)"
    # the four pair arrays alone are 10 bytes a row
    assert all(s >= 10 * R for R, s in sizes)
