"""ops.retrieve_topk's k range and the library's path / workspace answers, without a device."""
import pytest
import torch

import recsys_amd  # noqa: F401
from recsys_amd import _native as N
from recsys_amd import ops

# rsx_topk_path(Q, NI, k) for k <= 512 as the library answered before k > 512 existed
PATHS_K_LE_512 = [
    ((1, 1000, 10), 0), ((64, 5000, 100), 0), ((64, 16384, 100), 0), ((64, 16385, 100), 2), ((256, 47062, 500), 1),
    ((64, 100000, 20), 2), ((64, 100000, 512), 2), ((4096, 1000000, 100), 2), ((4096, 1000000, 512), 2),
    ((8192, 1000000, 500), 2), ((64, 20000, 512), 1), ((64, 32768, 512), 1), ((64, 65536, 512), 2),
    ((64, 65536, 300), 2), ((1, 262144, 1), 2), ((64, 17000, 200), 1),
]


@pytest.mark.parametrize("k,n_items", [(0, 5000), (2049, 5000), (2049, 1_000_000), (600, 599), (2048, 2047)])
def test_k_out_of_range_raises_before_any_device_work(k, n_items):
    U = torch.zeros(4, 128)
    I = torch.zeros(1, 128).expand(n_items, 128)      # only its shape is read before the refusal
    with pytest.raises(ValueError) as e:
        ops.retrieve_topk(U, I, k)                 # CPU tensors: a device call would raise RuntimeError
    assert str(ops.RETRIEVE_TOPK_MAX) in str(e.value) and "1 <= k" in str(e.value) and str(n_items) in str(e.value)


def test_max_k_matches_the_library():
    assert ops.RETRIEVE_TOPK_MAX == N.lib().rsx_topk_max_k() == 2048
    assert ops.RETRIEVE_TOPK_MAX <= ops.SELECT_TOPK_MAX          # the materialised route selects with it


def test_paths_for_k_up_to_512_are_unchanged():
    lib = N.lib()
    assert [(c, lib.rsx_topk_path(*c)) for c, _ in PATHS_K_LE_512] == PATHS_K_LE_512


@pytest.mark.parametrize("k", [513, 1000, 2048])
def test_large_k_paths_and_workspaces(k):
    lib = N.lib()
    assert lib.rsx_topk_path(64, 5000, k) == 3                   # not served natively
    assert lib.rsx_topk_path(64, 1_000_000, k) == lib.rsx_topk_path(4096, 1_000_000, k) == 2
    for fn in (lib.rsx_topk_workspace_bytes, lib.rsx_topk_workspace_bytes_corpus):
        sizes = [fn(q, 1_000_000, k) for q in (1, 64, 1000, 4096, 5000, 100_000)]
        assert all(s > 0 and s % 256 == 0 for s in sizes)
        assert sizes[0] <= sizes[1] <= sizes[2] <= sizes[3]
        assert sizes[3] == sizes[4] == sizes[5]                  # the 4096-query chunk bounds it
        assert fn(64, 5000, k) > 0 and fn(64, 5000, k) % 256 == 0
    # the exact fallback's score scratch is bounded whatever Q is: a few listed queries cost no more
    # than 256 MB beyond the scan's own buffers
    assert lib.rsx_topk_workspace_bytes_corpus(1, 1_000_000, k) <= (256 << 20) + (8 << 20)


def test_capacity_getters():
    lib = N.lib()
    assert lib.rsx_topk_stream_capacity() >= 8 and lib.rsx_topk_entry_capacity() >= 2 * 2048
    for k in (1, 512):
        assert lib.rsx_topk_margin_capacity(k) >= 2 * 512
    for k in (513, 2048):
        assert 2048 < lib.rsx_topk_margin_capacity(k) <= lib.rsx_topk_entry_capacity()
