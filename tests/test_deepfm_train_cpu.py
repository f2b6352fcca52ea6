"""CPU checks of the DeepFM training surface: the new entry points reject bad arguments before
any launch, unsupported shapes raise NotImplementedError, and the reference helper's float32 run
stays far inside the end-to-end cap of test_gpu_deepfm_train.py (the cap's premise)."""
import ctypes
import os

import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import _native
from recsys_amd.temp_model.ranker_skelet import DeepFM
from tests import deepfm_train_ref as REF


def _lib():
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built")
    return _native.load()


P = ctypes.c_void_p(16)   # a non-null pointer that is never dereferenced: every call below is rejected first


def test_training_entry_points_reject_bad_arguments():
    lib = _lib()
    vocab = _native.i64_array([10] * 65)
    arr = (ctypes.c_void_p * 65)(*([16] * 65))

    def err():
        return lib.rsx_last_error()

    assert lib.rsx_deepfm_train_keys(None, 4, 3, vocab, P, P, P, None) == 1 and b"null tensor" in err()
    assert lib.rsx_deepfm_train_keys(P, 4, 0, vocab, P, P, P, None) == 1 and b"F must be in [1,64]" in err()
    assert lib.rsx_deepfm_train_keys(P, 4, 65, vocab, P, P, P, None) == 1 and b"F must be in [1,64]" in err()
    assert lib.rsx_deepfm_train_segments(P, None, 4, P, P, None) == 1 and b"null tensor" in err()
    assert lib.rsx_deepfm_train_starts(None, 4, P, P, None) == 1 and b"null tensor" in err()
    assert (lib.rsx_deepfm_train_head(None, 128, P, P, None, P, 4, 1, P, P, P, P, 1 << 20, P, P, P, None) == 1
            and b"null tensor" in err())
    assert (lib.rsx_deepfm_train_head(P, 64, P, P, None, P, 4, 1, P, P, P, P, 1 << 20, P, P, P, None) == 1
            and b"128 wide" in err())
    assert lib.rsx_relu_bwd(None, P, 4, None) == 1 and b"null tensor" in err()
    assert lib.rsx_deepfm_train_contrib(P, P, None, 48, P, 4, 3, 16, P, P, None) == 1 and b"null tensor" in err()
    assert lib.rsx_deepfm_train_contrib(P, P, P, 48, P, 4, 65, 16, P, P, None) == 1 and b"F must be in [1,64]" in err()
    assert lib.rsx_deepfm_train_contrib(P, P, P, 24, P, 4, 3, 8, P, P, None) == 1 and b"embedding dim must be 16" in err()

    def adam(keys=P, F=3, E=16):
        return lib.rsx_deepfm_train_sparse_adam(keys, P, P, P, 12, F, E, vocab, P, P, arr, arr, arr, arr, arr, arr,
                                                1e-3, 0.9, 0.999, 1e-8, 1, P, 1 << 20, None, None, None)

    assert adam(keys=None) == 1 and b"null tensor" in err()
    assert adam(F=0) == 1 and b"F must be in [1,64]" in err()
    assert adam(F=65) == 1 and b"F must be in [1,64]" in err()
    assert adam(E=32) == 1 and b"embedding dim must be 16" in err()


def test_unsupported_shapes_raise():
    with pytest.raises(NotImplementedError, match="256, 128"):
        DeepFM([10] * 3, dnn_hidden_units=(64, 32)).make_trainer()
    with pytest.raises(NotImplementedError, match="F <= 64"):
        DeepFM([4] * 65).make_trainer()


@pytest.mark.parametrize("R,vocabs", [(77, [50] * 5), (1000, [500] * 39)])
def test_float32_reference_is_far_inside_the_cap(R, vocabs):
    """Three steps of the reference recipe in float32 against float64 (zero moments, fresh Zipf
    batches, lr 1e-2): no element of any parameter beyond 1e-3 lr and a loss difference under 1e-7, so
    the GPU test's cap (0.1 % of elements beyond 1e-2 lr) is left entirely to the code under test."""
    lr = 1e-2
    params = REF.make_params(vocabs, seed=4)
    r64 = REF.RefTrainer(params, lr=lr)
    r32 = REF.RefTrainer(params, lr=lr, dtype=torch.float32)
    for s in range(3):
        g = torch.Generator().manual_seed(20 + s)
        x, y = REF.zipf_ids(R, vocabs, g), REF.labels(R, g)
        l64, l32 = float(r64.step(x, y)), float(r32.step(x, y))
        print(f"step {s + 1}: float32 loss differs by {abs(l64 - l32):.2e}")
        assert abs(l64 - l32) < 1e-7
    worst = 0.0
    for (n, a), (_, b) in zip(REF.all_tensors(r32.p), REF.all_tensors(r64.p)):
        frac, mx = REF.cap_violations(a, b, lr)
        worst = max(worst, mx)
        assert mx <= 1e-3, f"{n}: float32 alone differs by {mx:.2e} lr"
    print(f"float32 vs float64 after 3 steps: largest difference {worst:.2e} lr")
