"""CPU checks of the ranker's training rows: the oracle tests/ranker_rows_ref.py against itself (the draw is
uniform over the non-bought items; the rank map at its edges), HMLogImporter's host half against the
reference's CSV semantics on a 30-line file, and the two native entry points' ABI (arity; argument checks
that return before any launch)."""
import os
import re

import numpy as np
import pytest

import recsys_amd  # noqa: F401
from recsys_amd import _native
from recsys_amd.utils.monitor.log_importer import HMLogImporter
from tests import ranker_rows_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_draw_is_uniform_over_the_items_not_bought():
    N, s, draws = 17, [0, 3, 4, 9, 16], 120000
    items = RR.draw(12345, np.arange(draws), s, N)
    eligible = [i for i in range(N) if i not in s]
    counts = np.bincount(items, minlength=N)
    assert counts[s].sum() == 0 and counts.sum() == draws          # every draw lands in the 12 eligible items
    p = 1.0 / len(eligible)
    sd = np.sqrt(draws * p * (1.0 - p))                            # binomial: 95.7
    dev = np.abs(counts[eligible] - draws * p).max() / sd
    print(f"largest deviation of a count from {draws * p:.0f}: {dev:.2f} standard deviations")
    assert dev <= 5.0


def test_hash_u32_equals_its_scalar_statement():
    def scalar(seed, idx):
        m = 0xFFFFFFFF
        x = (idx & m) ^ (((idx >> 32) * 0x9E3779B1) & m) ^ (seed & m)
        x ^= ((seed >> 32) * 0x85EBCA77) & m
        x ^= x >> 16
        x = (x * 0x85EBCA6B) & m
        x ^= x >> 13
        x = (x * 0xC2B2AE35) & m
        return x ^ (x >> 16)

    idx = np.asarray([0, 1, 2 ** 31, 2 ** 32 + 5, 2 ** 40 + 7, 123456789])
    for seed in (0, 42, 2 ** 63 + 12345, 2 ** 64 - 1):
        assert RR.hash_u32(seed, idx).tolist() == [scalar(seed, int(i)) for i in idx]


def test_the_rank_map_at_its_edges():
    N = 6
    assert RR.rank_map([0], np.arange(N - 1)).tolist() == [1, 2, 3, 4, 5]
    assert RR.rank_map([N - 1], np.arange(N - 1)).tolist() == [0, 1, 2, 3, 4]
    assert RR.rank_map(list(range(N - 1)), [0]).tolist() == [N - 1]
    assert RR.rank_map([], np.arange(N)).tolist() == list(range(N))
    rng = np.random.default_rng(0)
    for _ in range(20):                                            # a bijection [0, M) -> the complement, ascending
        s = np.sort(rng.permutation(40)[:rng.integers(0, 40)])
        want = [i for i in range(40) if i not in set(s.tolist())]
        assert RR.rank_map(s, np.arange(40 - len(s))).tolist() == want


LINES = [("c03", "a1"), ("c01", "a5"), ("c02", "zz"), ("c01", "a2"), ("c03", "a1"), ("c05", "a0"), ("c01", "zz"),
         ("c04", "a3"), ("c01", "a5"), ("c03", "a4"), ("c05", "a2"), ("c02", "yy"), ("c04", "a3"), ("c06", "a6"),
         ("c01", "a0"), ("c03", "a2"), ("c05", "a0"), ("c06", "a1"), ("c04", "a7"), ("c01", "a6"), ("c07", "xx"),
         ("c08", "a4"), ("c03", "a6"), ("c08", "a5"), ("c05", "a7"), ("c06", "a6"), ("c08", "a4"), ("c09", "a1"),
         ("c09", "a2"), ("c10", "a3")]
STORE_KEYS = ["a3", "a0", "a7", "a1", "a5", "a2", "a6", "a4", "a9"]       # key order, not sorted: a3 is item 0


def _write(tmp_path, lines):
    path = tmp_path / "transactions.csv"
    with open(path, "w") as f:
        f.write("t_dat,customer_id,article_id,price,sales_channel_id\n")
        for k, (c, a) in enumerate(lines):
            f.write(f"2020-01-{k % 28 + 1:02d},{c},{a},0.0{k},1\n")
    return str(path)


def test_read_log_keeps_the_references_csv_semantics(tmp_path):
    assert len(LINES) == 30
    store = {k: np.full(4, i, np.float32) for i, k in enumerate(STORE_KEYS)}
    imp = HMLogImporter(_write(tmp_path, LINES), store)
    for limit in (30, 12, 100000):
        log = imp.read_log(limit)
        by = {}
        for c, a in LINES[:limit]:
            by.setdefault(c, []).append(a)
        customers = sorted(by)
        assert log["customer_ids"].tolist() == customers                 # ascending customer_id
        want = [(g, STORE_KEYS.index(a)) for g, c in enumerate(customers) for a in by[c] if a in store]
        assert list(zip(log["pos_customer"].tolist(), log["pos_item"].tolist())) == want
        assert log["pos_customer"].dtype == log["pos_item"].dtype == log["bought"].dtype == np.int32
        assert log["bought_off"].dtype == np.int64 and len(log["bought_off"]) == len(customers) + 1
        for g, c in enumerate(customers):
            got = log["bought"][log["bought_off"][g]:log["bought_off"][g + 1]].tolist()
            assert got == sorted({STORE_KEYS.index(a) for a in by[c] if a in store}), c
    log = imp.read_log(30)
    groups = log["pos_customer"].tolist()
    assert 1 not in groups and 6 not in groups and max(groups) == 9     # c02, c07: all skipped, their ids stay unused
    assert groups.count(0) == 5                                          # c01: a5 twice, zz skipped
    assert log["pos_item"][:5].tolist() == [4, 5, 4, 1, 6]               # file order; an index is the key's position
    items, y, g = RR.importer(LINES, STORE_KEYS, 30, 2, 7)
    assert len(items) == 3 * len(groups) and y.reshape(-1, 3)[:, 0].all() and not y.reshape(-1, 3)[:, 1:].any()
    assert g.reshape(-1, 3)[:, 0].tolist() == groups


def test_the_native_entry_points_have_the_headers_arity_and_reject_bad_arguments_without_a_gpu():
    text = open(os.path.join(ROOT, "include", "recsys_amd.h")).read()
    for name in ("rsx_ranker_rows_sample", "rsx_pair_tabular"):
        m = re.search(r"^int\s+" + name + r"\(([^;]*?)\);", text, flags=re.M | re.S)
        assert m, name
        assert len(_native._SIGS[name][1]) == m.group(1).count(",") + 1, name
    if not os.path.exists(_native.LIB_PATH):
        pytest.skip("library not built")
    lib = _native.load()
    p = 16
    assert lib.rsx_ranker_rows_sample(p, p, 10, p, p, 4, 3, 5, 3, 42, p, p, p, None, None) == 1
    assert b"null tensor" in lib.rsx_last_error()
    assert lib.rsx_ranker_rows_sample(p, p, 10, p, p, 4, 3, 5, -1, 42, p, p, p, p, None) == 1 and b"K" in lib.rsx_last_error()
    assert lib.rsx_ranker_rows_sample(p, p, 1 << 29, p, p, 4, 3, 5, 3, 42, p, p, p, p, None) == 1
    assert b"2^31" in lib.rsx_last_error()
    assert lib.rsx_ranker_rows_sample(p, p, 10, p, p, 4, 0, 5, 3, 42, p, p, p, p, None) == 1
    assert lib.rsx_pair_tabular(p, p, None, p, p, p, p, 0, 3, 5, 8, None, None, 0, p, None, p, None) == 1
    assert b"R < 2^31" in lib.rsx_last_error()
    assert lib.rsx_pair_tabular(p, p, None, p, p, p, p, 4, 3, 5, 65537, None, None, 0, p, None, p, None) == 1
    assert lib.rsx_pair_tabular(p, p, None, p, p, p, p, 4, 3, 5, 8, None, None, 0, p, p, p, None) == 1
    assert b"truth_off" in lib.rsx_last_error()
    assert lib.rsx_pair_tabular(p, p, None, p, None, p, p, 4, 3, 5, 8, None, None, 0, p, None, p, None) == 1
