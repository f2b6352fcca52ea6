"""The towers' feature frames from the transaction log (reference staticstics/preprosess_agg_parallel.py, whose
spelling the path keeps): features_user_w_meta, features_item and features_sequence, which both FeatureProcessors
(tower_code/v1_refine_usertower.py, utils/data_preprocessing/feature_processor.py) read unchanged.

The reference runs pandas groupbys over the log and a pandarallel apply per customer. Here the log becomes a
TransactionTable on the device once (host half vectorised: factorise the ids, days since 1970-01-01, upload; one
stable device sort by (customer, day)) and every per-customer and per-item quantity is a segmented scan of
csrc/tx_features.hip (ops.tx_*; the specification is in include/recsys_amd.h, "transaction features"). The
functions keep the reference's names, take the transactions frame (t_dat, customer_id, article_id, price,
sales_channel_id) or a prepared TransactionTable, return frames with the reference's column names and dtypes and
write parquet only when a path is given. No module-level paths, no pandarallel.

Definitions where the reference leaves a choice ("transaction features"): rows of one customer and day
keep file order (it decides last_price and the order of same-day sequence entries); means are float64 (the
reference's float32 groupby.mean rounds them to float32); the qcut edges are pandas' bit for bit; a
validation subset selects rows of the full result, its statistics are not recomputed over the subset."""
from __future__ import annotations

import numpy as np
import pandas as pd
import pyarrow as pa
import torch

from .. import ops

TX_COLUMNS = ("t_dat", "customer_id", "article_id", "price", "sales_channel_id")
USER_FINAL_COLS = ["customer_id", "user_avg_price_bucket", "total_cnt_bucket", "recency_bucket", "age_bucket",
                   "price_std_scaled", "last_price_diff_scaled", "repurchase_ratio_scaled", "weekend_ratio_scaled",
                   "preferred_channel", "active_months", "FN", "Active", "club_member_status_idx",
                   "fashion_news_frequency_idx"]
USER_LEGACY_COLS = ["customer_id", "user_avg_price_log", "total_cnt_log", "repurchase_ratio", "recency_log",
                    "preferred_channel"]
ITEM_FINAL_COLS = ["article_id", "raw_probability", "pop_1w_log", "pop_1m_log", "velocity_1w", "velocity_1m",
                   "steady_score_log", "avg_item_price_log", "days_since_release_log"]
META_COLS = ["age_bucket", "FN", "Active", "club_member_status_idx", "fashion_news_frequency_idx"]


def days_since_epoch(t_dat) -> np.ndarray:
    """t_dat (datetimes or ISO strings) -> int32 days since 1970-01-01."""
    d = pd.to_datetime(pd.Series(np.asarray(t_dat))).to_numpy().astype("datetime64[D]")
    return (d - np.datetime64("1970-01-01", "D")).astype(np.int64).astype(np.int32)


def _id_column(col) -> np.ndarray:
    """The ids of a frame column as Python strings (an object array): strings pass, anything else is converted."""
    return col.to_numpy() if col.dtype == object else col.astype(str).to_numpy(dtype=object)


class TransactionTable:
    """The log on the device, sorted by (customer, day), same-day ties in file order: cust_off int64 [C + 1], item
    and day int32 [T], price fp32 [T], channel uint8 [T]; customer_ids / article_ids are the host id arrays in
    ascending order (row c / item i of every result). The derived columns and statistics are computed on first use
    and kept."""

    def __init__(self, cust_off, item, day, price, channel, customer_ids, article_ids):
        self.cust_off, self.item, self.day, self.price, self.channel = cust_off, item, day, price, channel
        self.customer_ids, self.article_ids = customer_ids, article_ids
        self.n_rows, self.n_customers, self.n_items = item.numel(), len(customer_ids), len(article_ids)
        self._cache = {}

    @classmethod
    def from_frame(cls, df, device=None):
        missing = [c for c in TX_COLUMNS if c not in df.columns]
        if missing:
            raise ValueError(f"TransactionTable.from_frame: the transactions frame lacks {missing}")
        if len(df) == 0:
            raise ValueError("TransactionTable.from_frame: the transactions frame is empty")
        dev = torch.device("cuda" if device is None else device)
        # ids are ordered as strings, what the frames hold: numeric ids are converted first
        cust, customer_ids = pd.factorize(_id_column(df["customer_id"]), sort=True)
        item, article_ids = pd.factorize(_id_column(df["article_id"]), sort=True)
        day = days_since_epoch(df["t_dat"])
        if int(day.min()) < 0:
            raise ValueError("TransactionTable.from_frame: a t_dat before 1970-01-01")
        cust_d = torch.from_numpy(cust.astype(np.int64)).to(dev)
        day_d = torch.from_numpy(day).to(dev)
        order = torch.sort((cust_d << 32) | day_d.to(torch.int64), stable=True).indices      # ties: file order
        cust_off = torch.zeros(len(customer_ids) + 1, device=dev, dtype=torch.int64)
        torch.cumsum(torch.bincount(cust_d, minlength=len(customer_ids)), 0, out=cust_off[1:])
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)[order].contiguous()      # noqa: E731
        return cls(cust_off, up(item.astype(np.int32)), day_d[order].contiguous(),
                   up(df["price"].to_numpy(dtype=np.float32)), up(df["sales_channel_id"].to_numpy(dtype=np.uint8)),
                   np.asarray(customer_ids), np.asarray(article_ids))

    def _get(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    @property
    def row_customer(self):
        """int32 [T]: the customer of every row."""
        return self._get("row_customer", lambda: ops.tx_segment_rows(self.cust_off, self.n_rows))

    @property
    def calendar(self):
        """(weekend uint8, month int32, week int32), each [T]."""
        return self._get("calendar", lambda: ops.tx_calendar(self.day))

    @property
    def max_day(self) -> int:
        return self._get("max_day", lambda: int(self.day.max()))

    def _sorted_within_customer(self, val):
        """val int32 [T] in ascending order inside every customer: one sort of the 64-bit key (customer, val)."""
        keys = torch.sort((self.row_customer.to(torch.int64) << 32) | val.to(torch.int64)).values
        return (keys & 0xFFFFFFFF).to(torch.int32)

    @property
    def items_by_customer(self):
        """int32 [T]: every customer's items in ascending order (the distinct items, the repurchase runs)."""
        return self._get("items_by_customer", lambda: self._sorted_within_customer(self.item))

    def customer_stats(self):
        """ops.tx_segment_stats per customer plus uniq (distinct items) and months (distinct months), int32 [C]."""
        def make():
            seg, C = self.row_customer, self.n_customers
            weekend, month, _ = self.calendar
            st = ops.tx_segment_stats(seg, C, self.price, self.day, self.channel, weekend)
            st["uniq"] = ops.tx_segment_distinct(seg, C, self.items_by_customer)
            st["months"] = ops.tx_segment_distinct(seg, C, month)
            return st
        return self._get("customer_stats", make)

    def item_stats(self):
        """ops.tx_segment_stats per item over the stable by-item order of the rows."""
        def make():
            weekend = self.calendar[0]
            by_item = torch.sort(self.item, stable=True)
            return ops.tx_segment_stats(by_item.values.contiguous(), self.n_items, self.price, self.day, self.channel,
                                        weekend, perm=by_item.indices.contiguous())
        return self._get("item_stats", make)

    def weekly_sales(self):
        """(weekly int32 [N, W], weeks int32 [W]): the reference's weekly pivot; weeks are Monday-start week numbers
        floor((day + 3) / 7), only those with a sale."""
        return self._get("weekly", lambda: ops.tx_weekly_sales(self.item, self.calendar[2], self.n_items))

    def item_features(self):
        """fp32 [8, N] in the order ops.TX_ITEM_COLUMNS."""
        def make():
            st = self.item_stats()
            return ops.tx_item_features(self.weekly_sales()[0], st["count"], st["sum"], st["dmin"], self.n_rows,
                                        self.max_day)
        return self._get("item_features", make)

    def user_features(self):
        """ops.tx_user_features of customer_stats(): (f64 [3, C], cols fp32 [11, C], channel int8, months int16)."""
        def make():
            st = self.customer_stats()
            return ops.tx_user_features(st, st["uniq"], st["months"], self.max_day)
        return self._get("user_features", make)

    def sequences(self, valid=None, max_len=50):
        """The CSR (seq_off int64 [C + 1], seq_item int32, seq_delta int32) of every customer's last max_len rows
        whose item is marked in valid (uint8 / bool [N], host or device; None: every item), on the device."""
        if valid is None:
            v = torch.ones(self.n_items, device=self.item.device, dtype=torch.uint8)
        else:
            v = torch.as_tensor(np.asarray(valid.cpu()) if torch.is_tensor(valid) else np.asarray(valid))
            v = v.to(torch.uint8).to(self.item.device).contiguous()
        if v.numel() != self.n_items:
            raise ValueError(f"TransactionTable.sequences: valid has {v.numel()} entries for {self.n_items} items")
        return ops.tx_sequences(self.row_customer, self.n_customers, self.item, self.day, v, max_len)

    def item_categories(self):
        """(item_cat int32 [N] on the device, the category codes): the reference's category_code = the first three
        characters of the article id. The ids ascend as strings, so a category's items are contiguous and item_cat
        does not decrease. Host work over the N items only."""
        def make():
            codes, cats = pd.factorize(pd.Series(_ids(self.article_ids)).str[:3].to_numpy(dtype=object))
            return torch.from_numpy(codes.astype(np.int32)).to(self.item.device), np.asarray(cats)
        return self._get("item_categories", make)

    def persona_features(self):
        """fp64 [7, C] in the order ops.PERSONA_COLUMNS, the behaviour columns of the reference's
        staticstics/preprocess_clustering.py:
          basket_size         the customer's rows n
          avg_price           sum / n
          cat_entropy         ln n - (sum n_c ln n_c) / n over the customer's category counts n_c (ops.tx_segment_runs
                              over the rows sorted by (customer, category)): scipy's entropy(value_counts), natural
                              log; 0 for a single category
          long_tail_ratio     the share of rows whose item is not a head item. Head items: the first max(int(0.2 N),
                              1) items by count descending, ties by ascending item index (the reference leaves
                              ties to pandas' value_counts; this is the project's definition)
          weekend_ratio       wkend / n
          repurchase_rate     the share of rows whose item the customer bought more than once (repeated / n of
                              ops.tx_segment_runs over (customer, item)). Not user_features()' repurchase_ratio =
                              1 - uniq / n, the share of rows beyond an item's first: for purchases a, a, a, b the
                              rate is 3/4 and the ratio 2/4. Both are kept, each for its reference module
          relative_price_pos  the mean over the customer's rows of price / the mean price of the item's category
        """
        def make():
            seg, C = self.row_customer, self.n_customers
            st, it = self.customer_stats(), self.item_stats()
            n = st["count"].to(torch.float64)
            per_row = lambda total: torch.where(n > 0, total / n, torch.zeros_like(n))      # noqa: E731
            item_cat, cats = self.item_categories()
            item_l = self.item.to(torch.int64)
            # categories per customer
            runs, _, nlogn = ops.tx_segment_runs(seg, C, self._sorted_within_customer(item_cat[item_l]))
            entropy = torch.where(runs > 1, torch.log(n) - nlogn / n, torch.zeros_like(n))
            # head items: one stable sort of the N counts
            n_head = max(int(0.2 * self.n_items), 1)
            is_tail = torch.ones(self.n_items, device=seg.device, dtype=torch.float64)
            is_tail[torch.sort(it["count"], descending=True, stable=True).indices[:n_head]] = 0.0
            tail_rows = ops.tx_segment_sum_f64(seg, C, is_tail[item_l].contiguous(), m2=False)[1]
            _, repeated, _ = ops.tx_segment_runs(seg, C, self.items_by_customer)
            # the category's mean price: its items' sums over its items' counts
            n_cat = len(cats)
            cat_sum = ops.tx_segment_sum_f64(item_cat, n_cat, it["sum"], m2=False)[1]
            cat_cnt = ops.tx_segment_sum_f64(item_cat, n_cat, it["count"].to(torch.float64), m2=False)[1]
            ratio = ops.tx_price_ratio(self.item, self.price, item_cat, cat_sum / cat_cnt)
            ratio_sum = ops.tx_segment_sum_f64(seg, C, ratio, m2=False)[1]
            return torch.stack([n, per_row(st["sum"]), entropy, per_row(tail_rows), per_row(st["wkend"].to(torch.float64)),
                                per_row(repeated.to(torch.float64)), per_row(ratio_sum)])
        return self._get("persona_features", make)

    def check(self):
        """Raise IndexError for any range error the kernels flagged so far (waits for their flags)."""
        for g in (ops._TX_CALENDAR_GUARD, ops._TX_ROWS_GUARD, ops._TX_STATS_GUARD, ops._TX_DISTINCT_GUARD,
                  ops._TX_WEEKLY_GUARD, ops._TX_SEQ_GUARD, ops._TX_RUNS_GUARD, ops._TX_SUM_GUARD, ops._TX_RATIO_GUARD):
            g.check()


def _table(src, device=None) -> TransactionTable:
    return src if isinstance(src, TransactionTable) else TransactionTable.from_frame(src, device)


def _save(df, save_path):
    if save_path is not None:
        df.to_parquet(save_path, index=False)
    return df


def _ids(a):
    return np.asarray(a).astype(str)


def _target_customers(target_val) -> np.ndarray:
    """The customers of a validation target: a parquet path or frame with customer_id, or the ids themselves."""
    if isinstance(target_val, str):
        target_val = pd.read_parquet(target_val)
    if isinstance(target_val, pd.DataFrame):
        target_val = target_val["customer_id"]
    return np.unique(_ids(list(target_val) if isinstance(target_val, (set, frozenset)) else target_val))


# ---------------------------------------------------------------------------------------------------------
def make_validation_target_file(full_df, valid_start_date, max_date, save_path=None):
    """The purchases of [valid_start_date, max_date] as one list per customer (:51-76): customer_id | target_ids.
    Plain pandas: it has no hot path."""
    t = pd.to_datetime(full_df["t_dat"])
    sub = full_df.loc[(t >= pd.to_datetime(valid_start_date)) & (t <= pd.to_datetime(max_date))]
    if sub.empty:
        return None
    truth = sub.groupby("customer_id")["article_id"].apply(list).reset_index()
    truth.columns = ["customer_id", "target_ids"]
    return _save(truth, save_path)


def make_item_features(train_df, save_path=None, device=None):
    """features_item (:168-240): article_id and the eight float32 columns, one row per article of the log in
    ascending id order."""
    tab = _table(train_df, device)
    cols = tab.item_features().cpu().numpy()
    tab.check()
    out = pd.DataFrame({"article_id": _ids(tab.article_ids)})
    for k, name in enumerate(ops.TX_ITEM_COLUMNS):
        out[name] = cols[k]
    return _save(out[ITEM_FINAL_COLS].fillna(0), save_path)


def customer_meta(customers, device=None) -> pd.DataFrame:
    """The customers.csv half of make_user_features (:356-379): a path or a frame -> customer_id and META_COLS
    (int8). Vectorised pandas on the host; only age_bucket goes through ops.quantile_bucket."""
    df = pd.read_csv(customers) if isinstance(customers, str) else customers.copy()
    if "postal_code" in df.columns:
        df = df.drop(columns=["postal_code"])
    age = df["age"].fillna(df["age"].median()).to_numpy(dtype=np.float64)
    dev = torch.device("cuda" if device is None else device)
    df["age_bucket"] = ops.quantile_bucket(torch.from_numpy(age).to(dev), 10).cpu().numpy()
    df["FN"] = df["FN"].fillna(0).astype(np.int8)
    df["Active"] = df["Active"].fillna(0).astype(np.int8)
    status = df["club_member_status"].fillna("OTHER").astype(str).str.upper()
    df["club_member_status_idx"] = status.map({"ACTIVE": 1, "PRE-CREATE": 2}).fillna(0).astype(np.int8)
    news = df["fashion_news_frequency"].fillna("NONE").astype(str).str.upper()
    df["fashion_news_frequency_idx"] = news.map({"REGULARLY": 1}).fillna(0).astype(np.int8)
    out = df[["customer_id"] + META_COLS].copy()
    out["customer_id"] = _ids(out["customer_id"])
    return out


def make_user_features(train_df, target_val_path=None, customers=None, save_path=None, device=None):
    """features_user_w_meta (:279-406): the bucket ids, the four standardised columns and the categorical ids of
    every customer of the log, ascending customer_id. target_val_path is accepted and ignored (the reference reads
    the file there and never uses it). customers: the customers.csv path or frame; without it the meta columns
    are 0, as the reference's left merge leaves a customer it does not know."""
    tab = _table(train_df, device)
    f64, cols, channel, months = tab.user_features()
    out = pd.DataFrame({"customer_id": _ids(tab.customer_ids)})
    for k, name in enumerate(("user_avg_price_bucket", "total_cnt_bucket", "recency_bucket")):
        out[name] = ops.quantile_bucket(f64[k].contiguous(), 10).cpu().numpy()
    c = cols.cpu().numpy()
    for name in ("price_std_scaled", "last_price_diff_scaled", "repurchase_ratio_scaled", "weekend_ratio_scaled"):
        out[name] = c[ops.TX_USER_COLUMNS.index(name)]
    out["preferred_channel"] = channel.cpu().numpy()
    out["active_months"] = months.cpu().numpy()
    tab.check()
    if customers is None:
        for name in META_COLS:
            out[name] = np.int8(0)
    else:
        out = pd.merge(out, customer_meta(customers, tab.item.device).drop_duplicates(subset=["customer_id"]),
                       on="customer_id", how="left")
        for name in META_COLS:
            out[name] = out[name].fillna(0).astype(np.int8)
    return _save(out[USER_FINAL_COLS].fillna(0), save_path)


def make_reranker_user_features(train_df, save_path=None, device=None):
    """The reranker's user frame (the reference's first make_user_features, :245-271, and :549-570): customer_id,
    user_avg_price_log, total_cnt_log, repurchase_ratio, recency_log (float32) and preferred_channel (int8)."""
    tab = _table(train_df, device)
    _, cols, channel, _ = tab.user_features()
    c = cols.cpu().numpy()
    tab.check()
    out = pd.DataFrame({"customer_id": _ids(tab.customer_ids)})
    for name in USER_LEGACY_COLS[1:5]:
        out[name] = c[ops.TX_USER_COLUMNS.index(name)]
    out["preferred_channel"] = channel.cpu().numpy()
    return _save(out[USER_LEGACY_COLS].fillna(0), save_path)


def make_validation_user_features(full_df, target_val_path, save_path=None, device=None):
    """make_reranker_user_features restricted to the customers of the validation target (:529-575)."""
    out = make_reranker_user_features(full_df, None, device)
    out = out[out["customer_id"].isin(_target_customers(target_val_path))].reset_index(drop=True)
    return _save(out, save_path)


def _valid_items(tab, processor) -> np.ndarray:
    ids = processor.item_ids if hasattr(processor, "item_ids") else processor
    return np.isin(_ids(tab.article_ids), _ids(list(ids)))


def make_cleaned_sequences(full_df, processor, save_path=None, max_len=50, device=None):
    """features_sequence (:410-469): per customer the last max_len purchases of an item the processor knows
    (processor.item_ids, or the ids themselves), oldest first: customer_id | sequence_ids (the article-id strings) |
    sequence_deltas (days before the customer's last kept purchase), each cell an array. A customer without such a
    purchase has no row."""
    tab = _table(full_df, device)
    seq_off, seq_item, seq_delta = tab.sequences(_valid_items(tab, processor), max_len)
    tab.check()
    off = seq_off.cpu().numpy()
    # the customers with an empty range have no row; the lists are built in one piece, not one customer at a time
    keep = np.flatnonzero(off[1:] > off[:-1])
    offsets = pa.array(off, type=pa.int64())
    ids = pa.DictionaryArray.from_arrays(pa.array(seq_item.cpu().numpy()), pa.array(_ids(tab.article_ids).tolist())).cast(pa.string())
    seqs = pa.table({"sequence_ids": pa.LargeListArray.from_arrays(offsets, ids),
                     "sequence_deltas": pa.LargeListArray.from_arrays(offsets, pa.array(seq_delta.cpu().numpy()))}).take(keep)
    out = seqs.to_pandas()
    out.insert(0, "customer_id", _ids(tab.customer_ids)[keep])
    return _save(out, save_path)


def make_validation_sequences(full_df, target_val_path, save_path=None, processor=None, max_len=50, device=None):
    """make_cleaned_sequences restricted to the customers of the validation target (:578-623); None when nothing is
    left, as the reference returns."""
    tab = _table(full_df, device)
    out = make_cleaned_sequences(tab, tab.article_ids if processor is None else processor, None, max_len)
    out = out[out["customer_id"].isin(_target_customers(target_val_path))].reset_index(drop=True)
    if out.empty:
        return None
    return _save(out, save_path)
