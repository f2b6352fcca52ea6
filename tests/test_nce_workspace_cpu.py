"""CPU checks of the contrastive-loss workspace layouts (csrc/nce_common.h: PlainLayout,
PlainX3Layout, GroupedLayout) through the three *_workspace_floats exports, and of the file list
behind the build stamp. The library loads without a GPU (tests/test_native_abi.py).

The tables below were recorded once from a library built at commit a561b91, the last one with the
single csrc/infonce.hip, whose entry points each derived their own offsets: the layouts must keep
every total, because callers size their buffers with them. rsx_nce_x3_workspace_floats depends on
the device's compute-unit count through its split rule; that count is 256 on an MI355X and 256 when
no device is found, so one table serves both machines."""
import glob
import os

import pytest

import recsys_amd  # noqa: F401
from recsys_amd import _native

NSPLIT_FWD = (1, 2, 8)
NSPLIT_BWD = 8
PRECISIONS = (0, 1, 2)  # fp32, bf16x3, f16

# (N, M): totals for nsplit_fwd = 1, 2, 8 (nsplit_bwd = 8)
PLAIN = {
    (0, 0): (16, 16, 16),
    (1, 1): (1048, 1052, 1076),
    (127, 127): (131080, 131588, 134636),
    (128, 128): (132112, 132624, 135696),
    (129, 129): (133144, 133660, 136756),
    (1029, 1029): (1061944, 1066060, 1090756),
    (5000, 5000): (5160016, 5180016, 5300016),
    (127, 1029): (1054728, 1055236, 1058284),
    (1029, 127): (1061944, 1066060, 1090756),
    (129, 5000): (5121048, 5121564, 5124660),
    (5000, 129): (5160016, 5180016, 5300016),
    (153151, 24442): (158051848, 158664452, 162340076),
    (24442, 153151): (157022176, 157119944, 157706552),
}
# (N, M): total (split counts from the library's own rule)
PLAIN_X3 = {
    (0, 0): 16,
    (1, 1): 464,
    (127, 127): 49808,
    (128, 128): 67088,
    (129, 129): 67664,
    (1029, 1029): 2440848,
    (5000, 5000): 11860048,
    (127, 1029): 416720,
    (1029, 127): 416336,
    (129, 5000): 1970128,
    (5000, 129): 1996560,
    (153151, 24442): 43560464,
    (24442, 153151): 42824144,
}
# (N, D): per precision (fp32, bf16x3, f16), totals for nsplit_fwd = 1, 2, 8 (nsplit_bwd = 8)
GROUPED = {
    (0, 0): ((64, 64, 64), (128, 128, 128), (128, 128, 128)),
    (1, 1): ((1088, 1088, 1088), (1408, 1408, 1408), (1408, 1408, 1408)),
    (127, 127): ((131136, 131648, 134656), (163712, 164224, 167232), (163712, 164224, 167232)),
    (128, 128): ((132160, 132672, 135744), (164992, 165504, 168576), (164992, 165504, 168576)),
    (129, 129): ((133184, 133696, 136768), (166272, 166784, 169856), (166272, 166784, 169856)),
    (1029, 1029): ((1061952, 1066112, 1090816), (1325440, 1329600, 1354304), (1325440, 1329600, 1354304)),
    (5000, 5000): ((5160064, 5180032, 5300032), (6440128, 6460096, 6580096), (6440128, 6460096, 6580096)),
    (127, 1029): ((1054784, 1055296, 1058304), (1202816, 1203328, 1206336), (1202816, 1203328, 1206336)),
    (1029, 127): ((1061952, 1066112, 1090816), (1209984, 1214144, 1238848), (1209984, 1214144, 1238848)),
    (129, 5000): ((5121088, 5121600, 5124672), (5777664, 5778176, 5781248), (5777664, 5778176, 5781248)),
    (5000, 129): ((5160064, 5180032, 5300032), (5816640, 5836608, 5956608), (5816640, 5836608, 5956608)),
    (153151, 24442): ((158051904, 158664512, 162340096), (180783872, 181396480, 185072064),
                      (180783872, 181396480, 185072064)),
    (24442, 153151): ((157022208, 157120000, 157706560), (179754176, 179851968, 180438528),
                      (179754176, 179851968, 180438528)),
}


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return _native.load()


def test_tables_cover_the_edge_sizes():
    sizes = {0, 1, 127, 128, 129, 1029, 5000}
    for table in (PLAIN, PLAIN_X3, GROUPED):
        assert {n for n, m in table if n == m} == sizes
        assert any(n < m for n, m in table) and any(n > m for n, m in table)
        assert (153151, 24442) in table  # the workload's own batch: rows x distinct targets


def test_plain_workspace_floats(lib):
    for (n, m), want in PLAIN.items():
        got = tuple(lib.rsx_nce_workspace_floats(n, m, nf, NSPLIT_BWD) for nf in NSPLIT_FWD)
        assert got == want, (n, m)


def test_plain_x3_workspace_floats(lib):
    for (n, m), want in PLAIN_X3.items():
        assert lib.rsx_nce_x3_workspace_floats(n, m) == want, (n, m)


def test_grouped_workspace_floats(lib):
    for (n, d), want in GROUPED.items():
        got = tuple(tuple(lib.rsx_nce_grouped_workspace_floats(n, d, nf, NSPLIT_BWD, pr) for nf in NSPLIT_FWD)
                    for pr in PRECISIONS)
        assert got == want, (n, d)


def test_stamp_covers_every_source_file():
    """An edit to any csrc/*.hip or csrc/*.h (the internal headers included) changes the build stamp."""
    files = _native.source_files()
    csrc = os.path.join(os.path.dirname(os.path.abspath(_native.__file__)), "csrc")
    on_disk = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")))
    assert on_disk and set(on_disk) <= set(files)
    names = [os.path.basename(f) for f in files]
    assert {"nce_common.h", "nce_mfma.h", "rsx_common.h", "nce_plain.hip", "nce_grouped.hip", "nce_grouped_f16.hip",
            "nce_emphasis.hip"} <= set(names)
    assert "infonce.hip" not in names
    assert names[-1] == "recsys_amd.h" and len(names) == len(set(names)) == len(on_disk) + 1
    # the Makefile's order: .hip sorted, then .h sorted, then the public header
    hips = [n for n in names if n.endswith(".hip")]
    hdrs = [n for n in names[:-1] if n.endswith(".h")]
    assert names == hips + hdrs + ["recsys_amd.h"]
    assert hips == sorted(hips, key=str.encode) and hdrs == sorted(hdrs, key=str.encode)
