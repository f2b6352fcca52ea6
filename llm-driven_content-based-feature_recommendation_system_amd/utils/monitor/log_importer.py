"""Drop-in for utils/monitor/log_importer.py: purchase logs -> the boosted ranker's training rows.

Reference (utils/monitor/log_importer.py:6-98): HMLogImporter reads the first `limit` lines of the
transactions CSV, walks the customers in ascending customer_id order and their purchases in file order, and
emits per purchase one positive row and negative_ratio rows of items drawn uniformly among those the
customer has not bought (a rejection loop over Python's random), all with a zero user vector; it returns
X_user, X_item, y, groups.

Here the host only factorises the CSV columns (pandas / numpy, no per-row Python): the positives in the
reference's order and each customer's distinct bought items as a CSR. The rows themselves are drawn on the
device by ops.ranker_sample_rows (rsx_ranker_rows_sample: the r-th non-bought item of a counter hash, no
rejection; include/recsys_amd.h, "ranker training rows") and stay there as a `RankerRows`, which
RecommendationRanker.train_rows turns into columns (ops.pair_tabular) and fits. Python's random stream is
not reproduced: the distribution is the reference's, the draws are not.
"""
from __future__ import annotations

import numpy as np
import torch

from ... import ops

_GROUP_MIX = (0x85EBCA6B, 0xC2B2AE35)     # the multipliers of hash_u32's finaliser (csrc/rsx_common.h)


class RankerRows:
    """(user, item) rows of the boosted ranker on one device: row_user, row_item int32 [R] (rows of the user
    and item vector tables), y fp32 [R] in {0, 1}, group_id int32 [R] (the rows of a group are one query) and
    score fp32 [R] or None (the retrieval score; None: the columns take the pair's dot product)."""

    def __init__(self, row_user, row_item, y, group_id, score=None):
        R = row_user.numel()
        for name, t in (("row_item", row_item), ("y", y), ("group_id", group_id), ("score", score)):
            if t is not None and t.numel() != R:
                raise ValueError(f"RankerRows: {name} holds {t.numel()} elements for {R} rows")
        self.row_user, self.row_item, self.y, self.group_id, self.score = row_user, row_item, y, group_id, score

    def __len__(self):
        return self.row_user.numel()

    def select(self, index):
        """The rows `index` (an int64 index or bool mask tensor on the rows' device)."""
        pick = lambda t: None if t is None else t[index].contiguous()   # noqa: E731
        return RankerRows(pick(self.row_user), pick(self.row_item), pick(self.y), pick(self.group_id), pick(self.score))

    def split(self, val_fraction, seed=0):
        """(training rows, validation rows): whole groups go to the validation side, those whose 32-bit hash
        of (group id, seed) falls below val_fraction 2^32, so a group's rows are never divided and the
        same group goes to the same side in every call. On the device; one host synchronisation (the sizes
        of the two sides)."""
        if not 0.0 <= val_fraction <= 1.0:
            raise ValueError(f"val_fraction must be in [0, 1] (got {val_fraction})")
        m = 0xFFFFFFFF
        x = (self.group_id.to(torch.int64) ^ (int(seed) & m)) & m
        x = ((x ^ (x >> 16)) * _GROUP_MIX[0]) & m
        x = ((x ^ (x >> 13)) * _GROUP_MIX[1]) & m
        x = x ^ (x >> 16)
        val = x < int(val_fraction * 4294967296.0)
        return self.select(~val), self.select(val)


class HMLogImporter:
    """Reference :6-98. item_vector_store: {article_id: vector}; an item's index is its position in the
    store's key order. The rows are built on `device` (default: the current GPU)."""

    def __init__(self, csv_path: str, item_vector_store: dict, device=None):
        self.csv_path = csv_path
        self.item_vector_store = item_vector_store
        self.all_product_ids = list(item_vector_store.keys())
        self._device = device

    @property
    def device(self):
        d = self._device
        return torch.device(d) if d is not None else torch.device("cuda", torch.cuda.current_device())

    def read_log(self, limit=100000):
        """The host half (vectorised): a dict of numpy arrays: pos_customer, pos_item int32 [Pv] = the valid
        positives in the reference's order (customers in ascending customer_id order, a customer's purchases
        in file order; a purchase of an article without a vector is skipped, a repeated purchase stays),
        pos_customer counting the customers of the first `limit` lines in that order (the reference's
        group_counter: it also counts a customer whose purchases were all skipped); bought_off int64 [C + 1]
        and bought int32 = each customer's distinct bought items with a vector, ascending; customer_ids [C]."""
        import pandas as pd
        df = pd.read_csv(self.csv_path, nrows=limit, usecols=["customer_id", "article_id", "t_dat"],
                         dtype={"article_id": str})
        n_items = len(self.all_product_ids)
        cust, customer_ids = pd.factorize(df["customer_id"], sort=True)
        C = len(customer_ids)
        item = pd.Index(self.all_product_ids).get_indexer(df["article_id"]) if n_items else np.full(len(df), -1)
        order = np.argsort(cust, kind="stable")          # ascending customers, file order within a customer
        cust, item = cust[order], item[order]
        keep = item >= 0
        pos_c, pos_i = cust[keep].astype(np.int64), item[keep].astype(np.int64)
        pairs = np.unique(pos_c * max(n_items, 1) + pos_i)          # distinct (customer, item), ascending
        b_c, b_i = pairs // max(n_items, 1), pairs % max(n_items, 1)
        off = np.zeros(C + 1, np.int64)
        np.cumsum(np.bincount(b_c, minlength=C), out=off[1:])
        return {"pos_customer": pos_c.astype(np.int32), "pos_item": pos_i.astype(np.int32), "bought_off": off,
                "bought": b_i.astype(np.int32), "customer_ids": np.asarray(customer_ids)}

    def load_rows(self, limit=100000, negative_ratio=5, seed=42, user_vectors=None, customer_index=None):
        """The reference's rows as a RankerRows on the device: per valid purchase the positive, then
        negative_ratio negatives (ops.ranker_sample_rows, a function of seed). group_id is the reference's
        group id. row_user is the row of the customer's vector: customer_index[customer_id] where
        customer_index (a mapping) is given, a customer it lacks being a KeyError; else the group id itself.
        user_vectors [C', d], when given, bounds row_user: ValueError for a row outside it. The row count is
        known from the host arrays: nothing is read back from the device (a range error is raised by
        ops._RANKER_ROWS_GUARD.check() or a later call)."""
        log = self.read_log(limit)
        dev, K = self.device, int(negative_ratio)
        C, Pv = len(log["customer_ids"]), len(log["pos_customer"])
        user_row = None
        if customer_index is not None:
            import pandas as pd
            keys = list(customer_index.keys())
            at = pd.Index(keys).get_indexer(log["customer_ids"]) if keys else np.full(C, -1)
            if (at < 0).any():
                raise KeyError(f"customer_index lacks {int((at < 0).sum())} of the log's {C} customers (the first: "
                               f"{log['customer_ids'][int(np.argmax(at < 0))]!r})")
            user_row = np.fromiter(customer_index.values(), np.int64, len(keys))[at]
        if user_vectors is not None:
            top = int(user_row.max()) if user_row is not None and C else C - 1
            low = int(user_row.min()) if user_row is not None and C else 0
            if low < 0 or top >= user_vectors.shape[0]:
                raise ValueError(f"the log's customers need user rows {low} .. {top}: user_vectors has "
                                 f"{user_vectors.shape[0]}")
        if Pv == 0:
            e32 = torch.empty(0, device=dev, dtype=torch.int32)
            return RankerRows(e32, e32.clone(), torch.empty(0, device=dev), e32.clone())
        up = lambda a: torch.from_numpy(a).to(dev)   # noqa: E731
        group, row_item, y = ops.ranker_sample_rows(up(log["pos_customer"]), up(log["pos_item"]), up(log["bought_off"]),
                                                    up(log["bought"]), len(self.all_product_ids), K, seed)
        row_user = group if user_row is None else up(user_row.astype(np.int32)).index_select(0, group.long())
        return RankerRows(row_user, row_item, y, group)

    def load_and_preprocess(self, limit=100000, negative_ratio=5, seed=42):
        """Reference :23-98, the same return value: X_user float32 [R, 128] zeros (the reference's
        default_user_vec), X_item float32 [R, d] = the store's vectors of the rows' items, y float32 [R],
        groups int32 [R], as host arrays."""
        rows = self.load_rows(limit, negative_ratio, seed)
        ops._RANKER_ROWS_GUARD.check()
        R = len(rows)
        if R == 0:
            empty = np.array([], dtype=np.float32)
            return empty, empty.copy(), empty.copy(), np.array([], dtype=np.int32)
        table = np.asarray(list(self.item_vector_store.values()), dtype=np.float32)
        X_item = table[rows.row_item.cpu().numpy()]
        return np.zeros((R, 128), np.float32), X_item, rows.y.cpu().numpy(), rows.group_id.cpu().numpy()
