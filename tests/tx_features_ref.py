"""The oracle of the transaction-feature tests: a pandas / numpy float64 restatement of the reference's
staticstics/preprosess_agg_parallel.py (make_item_features :168-240, make_user_features :279-406, the sequence
functions :410-469, the reranker's user frame :549-570) and of the specification in include/recsys_amd.h
("transaction features"). Nothing here imports the package.

Stated deviations from the reference, shared with the package: prices are the log's float32 values held
as float64 and every mean is float64 (the reference's float32 groupby.mean rounds the means to float32); rows of
one customer and day keep file order."""
import math

import numpy as np
import pandas as pd

ITEM_COLS = ("raw_probability", "pop_1w_log", "pop_1m_log", "velocity_1w", "velocity_1m", "steady_score_log",
             "avg_item_price_log", "days_since_release_log")
USER_FINAL_COLS = ["customer_id", "user_avg_price_bucket", "total_cnt_bucket", "recency_bucket", "age_bucket",
                   "price_std_scaled", "last_price_diff_scaled", "repurchase_ratio_scaled", "weekend_ratio_scaled",
                   "preferred_channel", "active_months", "FN", "Active", "club_member_status_idx",
                   "fashion_news_frequency_idx"]
USER_LEGACY_COLS = ["customer_id", "user_avg_price_log", "total_cnt_log", "repurchase_ratio", "recency_log",
                    "preferred_channel"]
META_COLS = ["age_bucket", "FN", "Active", "club_member_status_idx", "fashion_news_frequency_idx"]


# ---- calendar ----------------------------------------------------------------------------------------------
def calendar(day):
    """day (days since 1970-01-01, >= 0) -> (weekend, month = 12 year + month - 1, week = floor((day + 3) / 7))."""
    d = np.asarray(day, dtype=np.int64)
    z = d + 719468
    era = z // 146097
    doe = z - era * 146097
    yoe = (doe - doe // 1460 + doe // 36524 - doe // 146096) // 365
    doy = doe - (365 * yoe + yoe // 4 - yoe // 100)
    mp = (5 * doy + 2) // 153
    m = np.where(mp < 10, mp + 3, mp - 9)
    y = yoe + era * 400 + (m <= 2)
    return ((d + 3) % 7 >= 5).astype(np.uint8), (12 * y + m - 1).astype(np.int32), ((d + 3) // 7).astype(np.int32)


# ---- quantile buckets ----------------------------------------------------------------------------------------
def qcut_edges(x, q):
    """The distinct edges e_0 <= ... of the q-quantiles of x: e_k interpolates the sorted values at h = (n - 1) k / q,
    h formed in the float64 steps pandas' quantile takes (include/recsys_amd.h, "quantile buckets")."""
    s = np.sort(np.asarray(x, dtype=np.float64))
    n = len(s)
    edges = []
    step = np.float64(1.0) / np.float64(q)
    for k in range(q + 1):
        p = np.float64(1.0) if k == q else np.float64(k) * step      # np.linspace(0, 1, q + 1)[k]
        p = (p * np.float64(100.0)) / np.float64(100.0)              # pandas: np.percentile(values, qs * 100)
        h = np.float64(n - 1) * p                                     # numpy's virtual index of method 'linear'
        lo = int(np.floor(h))
        t = h - np.float64(lo)
        if lo >= n - 1:
            lo, t = n - 1, np.float64(0.0)
        a, b = s[lo], s[min(lo + 1, n - 1)]
        d = b - a
        e = b - d * (np.float64(1.0) - t) if t >= 0.5 else a + d * t
        if not edges or e != edges[-1]:
            edges.append(e)
    return np.asarray(edges, dtype=np.float64)


def qcut_bucket(x, q=10):
    """pd.qcut(x, q, labels=False, duplicates='drop') + 1 by the formula: #{edges < x}, at least 1."""
    x = np.asarray(x, dtype=np.float64)
    b = (qcut_edges(x, q)[None, :] < x[:, None]).sum(axis=1)
    return np.maximum(b, 1).astype(np.int8)


# ---- the sorted log ---------------------------------------------------------------------------------------------
def days_since_epoch(t_dat):
    d = pd.to_datetime(pd.Series(np.asarray(t_dat))).to_numpy().astype("datetime64[D]")
    return (d - np.datetime64("1970-01-01", "D")).astype(np.int64)


def prepare(df):
    """The log sorted by (customer_id, day), ties in file order, with day (int), price (the float32 value as
    float64), cust / item = the position of the id among the ascending distinct ids, and the calendar columns."""
    d = pd.DataFrame({"customer_id": np.asarray(df["customer_id"]).astype(str),
                      "article_id": np.asarray(df["article_id"]).astype(str),
                      "day": days_since_epoch(df["t_dat"]),
                      "price": df["price"].to_numpy(dtype=np.float32).astype(np.float64),
                      "channel": df["sales_channel_id"].to_numpy(dtype=np.int64)})
    customers, cust = np.unique(d["customer_id"].to_numpy(), return_inverse=True)
    articles, item = np.unique(d["article_id"].to_numpy(), return_inverse=True)
    d["cust"], d["item"] = cust, item
    order = np.lexsort((np.arange(len(d)), d["day"].to_numpy(), cust))
    d = d.iloc[order].reset_index(drop=True)
    d["weekend"], d["month"], d["week"] = calendar(d["day"].to_numpy())
    return d, customers, articles


def offsets(codes, n):
    off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(codes, minlength=n), out=off[1:])
    return off


def segment_stats(off, price, day, channel, weekend, perm=None):
    """Per segment [off[s], off[s + 1]) of the rows (read through perm when given): exact-sum float64 statistics."""
    price, day = np.asarray(price, dtype=np.float64), np.asarray(day, dtype=np.int64)
    channel, weekend = np.asarray(channel, dtype=np.int64), np.asarray(weekend, dtype=np.int64)
    S = len(off) - 1
    out = {"count": np.zeros(S, np.int64), "sum": np.zeros(S), "m2": np.zeros(S), "last": np.zeros(S),
           "dmin": np.zeros(S, np.int64), "dmax": np.zeros(S, np.int64), "chan": np.zeros(S, np.int64),
           "wkend": np.zeros(S, np.int64)}
    for s in range(S):
        rows = np.arange(off[s], off[s + 1])
        if perm is not None:
            rows = np.asarray(perm)[rows]
        if len(rows) == 0:
            continue
        p = price[rows]
        out["count"][s] = len(rows)
        out["sum"][s] = math.fsum(p)
        mean = out["sum"][s] / len(rows)
        out["m2"][s] = math.fsum((p - mean) ** 2)
        out["last"][s] = p[-1]
        out["dmin"][s], out["dmax"][s] = day[rows].min(), day[rows].max()
        out["chan"][s], out["wkend"][s] = channel[rows].sum(), (weekend[rows] != 0).sum()
    return out


def segment_distinct(off, val):
    val = np.asarray(val)
    return np.asarray([len(np.unique(val[off[s]:off[s + 1]])) for s in range(len(off) - 1)], dtype=np.int64)


# ---- items ---------------------------------------------------------------------------------------------------------
def weekly_sales(d, n_items):
    """The reference's pivot: (weekly int64 [N, W], the week numbers of its columns)."""
    week_start = d["day"] - (d["day"] + 3) % 7
    piv = d.groupby(["item", week_start]).size().unstack(fill_value=0).sort_index(axis=1)
    piv = piv.reindex(range(n_items), fill_value=0)
    return piv.to_numpy(dtype=np.int64), ((piv.columns.to_numpy(dtype=np.int64) + 3) // 7)


def item_columns(d, n_items, cold_days=14):
    """float64 [8, N] before the rounding to float32, imputation included (the imputed value is the mean of the
    float32 column), and is_new."""
    T = len(d)
    w, _ = weekly_sales(d, n_items)
    w = w.astype(np.float64)
    W = w.shape[1]
    st = segment_stats(offsets(d["item"].to_numpy(), n_items), d["price"], d["day"], d["channel"], d["weekend"],
                       perm=np.argsort(d["item"].to_numpy(), kind="stable"))
    n = st["count"].astype(np.float64)
    cur_w, prev_w = w[:, -1], (w[:, -2] if W > 1 else np.zeros(n_items))
    cur_m, prev_m = w[:, -4:].sum(axis=1), w[:, -8:-4].sum(axis=1)
    rec = w[:, -12:]
    k = rec.shape[1]
    mean = rec.sum(axis=1) / k
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.sqrt(((rec - mean[:, None]) ** 2).sum(axis=1) / (k - 1)) if k > 1 else np.full(n_items, np.nan)
        steady = np.nan_to_num(np.log1p(mean / (std + 1e-9)), nan=0.0)
    days = (d["day"].max() - st["dmin"]).astype(np.float64)
    cols = np.stack([n / T, np.log1p(cur_w), np.log1p(w[:, -4:].sum(axis=1)),
                     np.clip((cur_w - prev_w) / (prev_w + 1), -1, 5), np.clip((cur_m - prev_m) / (prev_m + 1), -1, 5),
                     steady, np.log1p(st["sum"] / n), np.log1p(days)])
    is_new = days < cold_days
    for c in (1, 2, 3, 4):
        cols[c, is_new] = math.fsum(cols[c].astype(np.float32).astype(np.float64)) / n_items
    return cols, is_new


def item_frame(df):
    d, _, articles = prepare(df)
    cols, _ = item_columns(d, len(articles))
    out = pd.DataFrame({"article_id": articles})
    for k, name in enumerate(ITEM_COLS):
        out[name] = cols[k].astype(np.float32)
    return out


# ---- users ---------------------------------------------------------------------------------------------------------
def user_columns(d, n_customers):
    """Everything make_user_features derives per customer, float64 before any rounding except where the reference
    standardises a float32 column (then the float32 value, as float64)."""
    off = offsets(d["cust"].to_numpy(), n_customers)
    st = segment_stats(off, d["price"], d["day"], d["channel"], d["weekend"])
    n = st["count"].astype(np.float64)
    by_item = d.sort_values(["cust", "item"], kind="stable")
    uniq = segment_distinct(off, by_item["item"].to_numpy()).astype(np.float64)
    months = segment_distinct(off, d["month"].to_numpy())
    mean = st["sum"] / n
    with np.errstate(invalid="ignore", divide="ignore"):
        std = np.where(n > 1, np.sqrt(st["m2"] / np.maximum(n - 1, 1)), 0.0)
    rec = (d["day"].max() - st["dmax"]).astype(np.float64)
    out = {"user_avg_price": mean, "total_cnt": n, "recency_days": rec, "price_std": std,
           "last_price_diff": st["last"] - mean, "repurchase_ratio": 1.0 - uniq / n, "weekend_ratio": st["wkend"] / n,
           "preferred_channel": np.where(st["chan"] / n > 1.5, 2, 1).astype(np.int8), "active_months": months.astype(np.int16),
           "user_avg_price_log": np.log1p(mean), "total_cnt_log": np.log1p(n), "recency_log": np.log1p(rec)}
    C = n_customers
    for name in ("price_std", "last_price_diff", "repurchase_ratio", "weekend_ratio"):
        x = out[name] if name == "weekend_ratio" else out[name].astype(np.float32).astype(np.float64)
        if C > 1:
            m = math.fsum(x) / C
            sd = math.sqrt(math.fsum((x - m) ** 2) / (C - 1))
            out[name + "_scaled"] = (x - m) / (sd + 1e-9)
        else:
            out[name + "_scaled"] = np.zeros(C)
    return out


def customer_meta(customers, bucket=qcut_bucket):
    df = customers.copy()
    if "postal_code" in df.columns:
        df = df.drop(columns=["postal_code"])
    df["age_bucket"] = bucket(df["age"].fillna(df["age"].median()).to_numpy(dtype=np.float64), 10)
    df["FN"] = df["FN"].fillna(0).astype(np.int8)
    df["Active"] = df["Active"].fillna(0).astype(np.int8)
    status = df["club_member_status"].fillna("OTHER").astype(str).str.upper()
    df["club_member_status_idx"] = status.map({"ACTIVE": 1, "PRE-CREATE": 2}).fillna(0).astype(np.int8)
    news = df["fashion_news_frequency"].fillna("NONE").astype(str).str.upper()
    df["fashion_news_frequency_idx"] = news.map({"REGULARLY": 1}).fillna(0).astype(np.int8)
    df["customer_id"] = df["customer_id"].astype(str)
    return df[["customer_id"] + META_COLS]


def user_frame(df, customers=None):
    d, cust_ids, _ = prepare(df)
    u = user_columns(d, len(cust_ids))
    out = pd.DataFrame({"customer_id": cust_ids})
    out["user_avg_price_bucket"] = qcut_bucket(u["user_avg_price"])
    out["total_cnt_bucket"] = qcut_bucket(u["total_cnt"])
    out["recency_bucket"] = qcut_bucket(u["recency_days"])
    for name in ("price_std_scaled", "last_price_diff_scaled", "repurchase_ratio_scaled", "weekend_ratio_scaled"):
        out[name] = u[name].astype(np.float32)
    out["preferred_channel"], out["active_months"] = u["preferred_channel"], u["active_months"]
    if customers is None:
        for name in META_COLS:
            out[name] = np.int8(0)
    else:
        out = pd.merge(out, customer_meta(customers).drop_duplicates(subset=["customer_id"]), on="customer_id", how="left")
        for name in META_COLS:
            out[name] = out[name].fillna(0).astype(np.int8)
    return out[USER_FINAL_COLS]


def legacy_user_frame(df):
    d, cust_ids, _ = prepare(df)
    u = user_columns(d, len(cust_ids))
    out = pd.DataFrame({"customer_id": cust_ids})
    for name in USER_LEGACY_COLS[1:5]:
        out[name] = u[name].astype(np.float32)
    out["preferred_channel"] = u["preferred_channel"]
    return out


# ---- sequences -------------------------------------------------------------------------------------------------------
def sequences(d, n_customers, valid, max_len=50):
    """Per customer (items, deltas) of the last max_len rows with valid[item], in the prepared order."""
    valid = np.asarray(valid, dtype=bool)
    off = offsets(d["cust"].to_numpy(), n_customers)
    item, day = d["item"].to_numpy(), d["day"].to_numpy()
    out = []
    for c in range(n_customers):
        rows = np.arange(off[c], off[c + 1])
        rows = rows[valid[item[rows]]][-max_len:]
        out.append((item[rows], (day[rows[-1]] - day[rows]) if len(rows) else day[rows]))
    return out


def sequence_frame(df, valid_ids, max_len=50):
    d, cust_ids, articles = prepare(df)
    seqs = sequences(d, len(cust_ids), np.isin(articles, np.asarray(list(valid_ids)).astype(str)), max_len)
    keep = [c for c, (i, _) in enumerate(seqs) if len(i)]
    return pd.DataFrame({"customer_id": cust_ids[keep],
                         "sequence_ids": [articles[seqs[c][0]].tolist() for c in keep],
                         "sequence_deltas": [seqs[c][1].tolist() for c in keep]})


# ---- test data -------------------------------------------------------------------------------------------------------
BASE_MONDAY = "2019-09-23"


def synth_log(n_customers, n_items, weeks, n_rows, seed, dyadic=True):
    """A shuffled log over the calendar weeks `weeks` (offsets from BASE_MONDAY; a week left out has no sale at
    all): skewed item popularity, every listed week and the last week's Sunday bought in, same-day repeat
    purchases, prices on the 2^-10 grid (dyadic) or arbitrary float32. Two more articles are first sold 13 and 14
    days before the last day."""
    rng = np.random.default_rng(seed)
    weeks = np.asarray(weeks)
    week = np.concatenate([weeks, rng.choice(weeks, n_rows - len(weeks))])
    dow = rng.integers(0, 7, n_rows)
    week[0], dow[0] = weeks[-1], 6                                      # the last day: the last week's Sunday
    day = week * 7 + dow
    cust = rng.integers(0, n_customers, n_rows)
    cust[rng.random(n_rows) < 0.15] = 0                                 # one customer with many rows
    item = np.minimum((n_items * rng.random(n_rows) ** 2.5).astype(np.int64), n_items - 1)
    price = rng.integers(1, 1 << 9, n_rows) / 1024.0 if dyadic else rng.gamma(2.0, 0.015, n_rows)
    channel = rng.integers(1, 3, n_rows)
    last = day.max()
    extra = [(last - 13, 1, "new13"), (last - 13, 2, "new13"), (last - 14, 1, "new14"), (last - 1, 3, "new14")]
    extra = [e for e in extra if (e[0] // 7) in set(weeks.tolist())]
    df = pd.DataFrame({"t_dat": np.datetime64(BASE_MONDAY, "D") + np.concatenate([day, [e[0] for e in extra]]).astype("timedelta64[D]"),
                       "customer_id": [f"c{c:05d}" for c in np.concatenate([cust, [e[1] for e in extra]])],
                       "article_id": [f"{700000 + i}" for i in item] + [{"new13": "0900013", "new14": "0900014"}[e[2]] for e in extra],
                       "price": np.concatenate([price, np.full(len(extra), 0.25)]).astype(np.float32),
                       "sales_channel_id": np.concatenate([channel, np.ones(len(extra), dtype=np.int64)]).astype(np.int8)})
    return df.iloc[rng.permutation(len(df))].reset_index(drop=True)


def ulps32(a, b):
    """The distance of two float32 arrays in units in the last place."""
    def ordered(x):
        i = np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(ordered(a) - ordered(b))
