"""Drop-in for gnn_model/v1_lightgcl.py: the LightGCL collaborative-filtering model, its graph build
and its training step.

Reference (gnn_model/v1_lightgcl.py): TrainDataset :65-99, build_graph :104-139, LightGCL :144-219, the
loop body of train :265-289.
Compute: the normalised adjacency A^ = D^-1/2 B D^-1/2 is never stored. NormAdjacency keeps the binary
CSR of B, deg^-1/2 and a static chunk plan for the long rows; torch.sparse.mm(adj, x) (:171) and its
backward are rsx_spmm_norm (ops.lightgcl_propagate: Horner over the layers, nothing saved for autograd),
the SVD view (:175-185) is rsx_lowrank_proj + q x q algebra + rsx_lowrank_update
(ops.lightgcl_global_rows, only the rows the loss reads), the two InfoNCE terms are the plain NCE
kernels (ops.nce_sum) with fp32 products over rows from rsx_gather_rows. fp32 throughout, no AMP; every sum in a fixed
order, so a step is reproducible bit for bit. There is no CPU path: the module constructs on CPU, the
ops raise on non-ROCm tensors.
"""
from __future__ import annotations

import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.data as data

from .. import ops

SPMM_CHUNK = ops.SPMM_CHUNK


def chunk_plan(row_ptr, chunk=SPMM_CHUNK):
    """The static plan of rsx_spmm_norm's long rows: (long_rows [L] ascending, part_off [L + 1],
    chunk_beg [C], chunk_end [C]), all int64. A row with more than `chunk` neighbours is cut into
    chunks of `chunk` CSR positions (the last one shorter); row l owns the partial slots
    [part_off[l], part_off[l + 1]), slot s covers the positions [chunk_beg[s], chunk_end[s])."""
    dev = row_ptr.device
    deg = row_ptr[1:] - row_ptr[:-1]
    long_rows = torch.nonzero(deg > chunk).reshape(-1)
    nch = (deg[long_rows] + chunk - 1) // chunk
    part_off = torch.zeros(long_rows.numel() + 1, dtype=torch.int64, device=dev)
    part_off[1:] = torch.cumsum(nch, 0)
    owner = torch.repeat_interleave(torch.arange(long_rows.numel(), device=dev), nch)
    k = torch.arange(owner.numel(), device=dev) - part_off[owner]
    chunk_beg = row_ptr[long_rows[owner]] + chunk * k
    chunk_end = torch.minimum(chunk_beg + chunk, row_ptr[long_rows[owner] + 1])
    return long_rows, part_off, chunk_beg, chunk_end


class NormAdjacency:
    """The user-item graph of LightGCL as rsx_spmm_norm reads it: the CSR of the binary symmetric
    bipartite matrix B over n = num_users + num_items nodes (users first; row_ptr int64 [n + 1], col
    int32 [nnz] ascending within a row), dinv fp32 [n] = deg^-1/2 (0 for an isolated node, the
    reference's inf -> 0 rule, :124-125) and the long-row chunk plan. Neither A^ = diag(dinv) B diag(dinv)
    nor its values are stored; to_sparse_coo() builds the reference's tensor on request. K = V^T U of the
    graph's SVD factors is attached by build_graph."""

    _TENSORS = ("row_ptr", "col", "dinv", "long_rows", "part_off", "chunk_beg", "chunk_end", "K")

    def __init__(self, edge_index, num_users, num_items, device=None, chunk=SPMM_CHUNK):
        num_users, num_items = int(num_users), int(num_items)
        n = num_users + num_items
        if n >= 2 ** 31:
            raise ValueError("NormAdjacency: column indices are int32, the graph has too many nodes")
        e = torch.as_tensor(edge_index)
        if e.dim() != 2 or e.shape[0] != 2:
            raise ValueError(f"NormAdjacency: edge_index must be [2, E], got {tuple(e.shape)}")
        if device is not None:
            e = e.to(device)
        u, i = e[0].long(), e[1].long()
        if e.shape[1] and (int(u.min()) < 0 or int(u.max()) >= num_users or int(i.min()) < 0
                           or int(i.max()) >= num_items):
            raise ValueError("NormAdjacency: edge_index holds a user or item outside the graph")
        # duplicate edges removed as torch.unique(edge_index, dim=1) does (:52); sorted by (user, item)
        key = torch.unique(u * num_items + i)
        u, i = key // num_items, key % num_items
        # the item rows: the same edges sorted by (item, user)
        key_t = torch.sort(i * num_users + u).values
        deg = torch.cat([torch.bincount(u, minlength=num_users), torch.bincount(i, minlength=num_items)])
        self.num_users, self.num_items, self.n, self.chunk = num_users, num_items, n, int(chunk)
        self.row_ptr = torch.zeros(n + 1, dtype=torch.int64, device=key.device)
        self.row_ptr[1:] = torch.cumsum(deg, 0)
        self.col = torch.cat([i + num_users, key_t % max(num_users, 1)]).to(torch.int32)
        dinv = deg.double().pow(-0.5)
        self.dinv = torch.where(deg > 0, dinv, torch.zeros_like(dinv)).float()
        self.long_rows, self.part_off, self.chunk_beg, self.chunk_end = chunk_plan(self.row_ptr, self.chunk)
        self.K = None
        self._ws = {}

    @property
    def nnz(self):
        return self.col.numel()

    @property
    def device(self):
        return self.row_ptr.device

    def to(self, device):
        """The same graph with its arrays on `device` (self when they already are)."""
        device = torch.device(device)
        if device == self.row_ptr.device:
            return self
        out = object.__new__(NormAdjacency)
        out.__dict__.update(self.__dict__)
        for name in self._TENSORS:
            t = getattr(self, name)
            setattr(out, name, None if t is None else t.to(device))
        out._ws = {}
        return out

    def workspace_bytes(self, D):
        """rsx_spmm_norm_workspace_bytes: one [D] fp32 partial slot per chunk of the plan."""
        return self.chunk_beg.numel() * int(D) * 4

    def workspace(self, D):
        """The partial-slot workspace for rows of D columns (None without long rows), allocated once."""
        if self.chunk_beg.numel() == 0:
            return None
        ws = self._ws.get(D)
        if ws is None:
            ws = self._ws[D] = torch.empty(self.workspace_bytes(D), dtype=torch.uint8, device=self.row_ptr.device)
        return ws

    def rows_of_edges(self):
        """The CSR row of every stored entry, int64 [nnz]."""
        deg = self.row_ptr[1:] - self.row_ptr[:-1]
        return torch.repeat_interleave(torch.arange(self.n, device=self.row_ptr.device), deg)

    def to_sparse_coo(self):
        """The reference's adj_tensor (:131-135): coalesced fp32 COO of A^, values dinv_r dinv_c."""
        r, c = self.rows_of_edges(), self.col.long()
        vals = self.dinv[r] * self.dinv[c]
        return torch.sparse_coo_tensor(torch.stack([r, c]), vals, (self.n, self.n)).coalesce()


class LowRankView:
    """The rank-q factors of A^ (U [n, q], S [q], V [n, q] of torch.svd_lowrank) with K = V^T U [q, q]:
    (U S V^T)^j E = U C_j with C_1 = S.(V^T E), C_{j+1} = S.(K C_j). U = +-V is not assumed."""

    def __init__(self, U, S, V, K=None):
        self.U, self.S, self.V = U.float().contiguous(), S.float().contiguous(), V.float().contiguous()
        self.K = (self.V.t() @ self.U) if K is None else K.float()

    def to(self, device):
        device = torch.device(device)
        if device == self.U.device:
            return self
        return LowRankView(self.U.to(device), self.S.to(device), self.V.to(device), self.K.to(device))


def build_graph(edge_index, num_users, num_items, device, q=5):
    """(adj, U, S, V) as the reference's build_graph (:104-139): adj is a NormAdjacency on `device`,
    U, S, V = torch.svd_lowrank(adj.to_sparse_coo(), q=q, niter=2); K = V^T U is kept on adj.K.
    Set-up code: the structure comes from torch sorts and counts on `device`."""
    adj = NormAdjacency(edge_index, num_users, num_items, device=device)
    U, S, V = torch.svd_lowrank(adj.to_sparse_coo(), q=q, niter=2)
    adj.K = V.t() @ U
    return adj, U, S, V


class TrainDataset(data.Dataset):
    """The reference's (user, positive item, sampled negative item) dataset (:65-99) with a vectorised
    sampler: sample_batch draws uniform items and redraws the ones that are an edge of their user,
    tested by searchsorted on the sorted user * num_items + item keys."""

    def __init__(self, edge_index, num_users, num_items):
        self.num_users = int(num_users)
        self.num_items = int(num_items)
        self.users = edge_index[0]
        self.items = edge_index[1]
        self.keys = torch.unique(self.users.long() * self.num_items + self.items.long())
        full = torch.bincount(self.keys // self.num_items, minlength=1) >= self.num_items
        if bool(full.any()):
            raise ValueError(f"TrainDataset: user {int(torch.nonzero(full)[0])} interacted with every item, "
                             "so no negative item exists for it")

    def __len__(self):
        return len(self.users)

    def _is_edge(self, users, items):
        key = users * self.num_items + items
        pos = torch.searchsorted(self.keys, key).clamp(max=max(self.keys.numel() - 1, 0))
        return self.keys[pos] == key if self.keys.numel() else torch.zeros_like(key, dtype=torch.bool)

    def sample_batch(self, idx, generator=None):
        """(users, pos_items, neg_items) int64 for the edges idx; generator: a torch.Generator on the
        edges' device (None: the default one)."""
        idx = torch.as_tensor(idx, device=self.users.device)
        users, pos = self.users[idx].long(), self.items[idx].long()
        neg = torch.randint(0, self.num_items, users.shape, generator=generator, device=users.device)
        while True:
            again = torch.nonzero(self._is_edge(users, neg)).reshape(-1)
            if again.numel() == 0:
                return users, pos, neg
            neg[again] = torch.randint(0, self.num_items, again.shape, generator=generator, device=users.device)

    def __getitem__(self, idx):
        u, p, n = self.sample_batch(torch.as_tensor([int(idx)]))
        return int(u), int(p), int(n)


class LightGCL(nn.Module):
    """The reference's module surface (:144-219): constructor arguments, the attributes num_users,
    num_items, emb_dim, n_layers, temp, lambda_ssl, adj, U, S, V, and the two tables embedding_user /
    embedding_item, the only state_dict entries. Both nn.Embedding are built before either gets its
    xavier_uniform_, user first: one seed then gives the reference's weights."""

    def __init__(self, num_users, num_items, config, adj_tensor, svd_components):
        super().__init__()
        if config["temp"] < 0.01:
            # the reference clamps logits at 100 (:207); on unit rows that needs 1 / temp > 100
            raise ValueError(f"LightGCL: temp = {config['temp']} < 0.01 would need the reference's logit clamp, "
                             "which the loss kernels do not apply")
        if not isinstance(adj_tensor, NormAdjacency):
            raise TypeError("LightGCL: adj_tensor must be the NormAdjacency that build_graph returns")
        self.num_users, self.num_items = num_users, num_items
        self.emb_dim, self.n_layers = config["emb_dim"], config["n_layers"]
        self.temp, self.lambda_ssl = config["temp"], config["lambda_ssl"]
        self.lambda_reg = config.get("lambda_reg", 0.0)   # train_step's weight of get_l2_reg
        self.adj = adj_tensor
        self.view = LowRankView(*svd_components)
        self.U, self.S, self.V = svd_components
        tables = [nn.Embedding(rows, self.emb_dim) for rows in (num_users, num_items)]
        self.embedding_user, self.embedding_item = tables
        for table in tables:
            nn.init.xavier_uniform_(table.weight)

    def _apply(self, fn, *args, **kwargs):
        """model.to(device) also moves the graph and the SVD factors (plain attributes, as in the
        reference, so the state_dict holds the two tables only)."""
        super()._apply(fn, *args, **kwargs)
        device = self.embedding_user.weight.device
        self.adj = self.adj.to(device)
        self.view = self.view.to(device)
        self.U, self.S, self.V = self.view.U, self.view.S, self.view.V
        return self

    @staticmethod
    def _check_ids(*pairs):
        """IndexError, as nn.Embedding raises it, if any index tensor leaves [0, rows): the row kernels
        take in-range indices only. pairs: (indices, rows). One host read for all of them."""
        bad = None
        for idx, rows in pairs:
            b = ((idx < 0) | (idx >= rows)).any()
            bad = b if bad is None else bad | b
        if bool(bad):
            raise IndexError("LightGCL: a user or item index is out of range")

    def all_embeddings(self):
        return torch.cat([self.embedding_user.weight, self.embedding_item.weight])

    def forward(self):
        """(local_final, global_final), both [num_users + num_items, emb_dim] (:163-186)."""
        all_emb = self.all_embeddings()
        local_final = ops.lightgcl_propagate(all_emb, self.adj, self.n_layers)
        global_final = ops.lightgcl_global_rows(all_emb, self.view, None, self.n_layers)
        return local_final, global_final

    @staticmethod
    def _bpr(u, p, n):
        """-mean log(sigmoid(<u, p> - <u, n>) + 1e-10), the reference's form (:192-194)."""
        margin = (u * p).sum(1) - (u * n).sum(1)
        return -(torch.sigmoid(margin) + 1e-10).log().mean()

    def calc_bpr_loss(self, local_emb, users, pos_items, neg_items):
        b = users.numel()
        self._check_ids((users, local_emb.shape[0]), (pos_items, local_emb.shape[0]), (neg_items, local_emb.shape[0]))
        rows = ops.gather_rows_sorted(local_emb, torch.cat([users, pos_items, neg_items]))
        return self._bpr(rows[:b], rows[b:2 * b], rows[2 * b:])

    def _info_nce(self, v1, v2):
        """F.cross_entropy(v1 @ v2.T / temp, arange) of L2-normalised rows (:203-209); the NCE kernels
        take 128 columns, narrower rows are zero-padded (every dot product unchanged).
        The plain kernels run here with fp32 products (the mode is read by the forward and kept for its
        backward): with the bf16x3 products the SSL gradient is off by 3e-5 of the tables' gradient scale,
        which three Adam steps turn into parameter deviations above 1e-5; fp32 products leave 1e-6."""
        if v1.shape[1] < 128:
            v1 = F.pad(v1, (0, 128 - v1.shape[1]))
            v2 = F.pad(v2, (0, 128 - v2.shape[1]))
        prev = ops.set_nce_precision("fp32")
        try:
            total, cnt = ops.nce_sum(v1, v2, tau=self.temp, flags=ops.NCE_PLAIN, precision=None, tag="lightgcl_ssl")
        finally:
            ops.set_nce_precision(prev)
        return total / cnt.clamp(min=1.0)

    def calc_ssl_loss(self, local_emb, global_emb, users, items):
        self._check_ids((users, local_emb.shape[0]), (items, local_emb.shape[0]))
        unique_users = torch.unique(users)
        unique_items = torch.unique(items)
        loss = 0.0
        for idx in (unique_users, unique_items):
            loss = loss + self._info_nce(ops.gather_rows(local_emb, idx, normalize=True, unique=True),
                                         ops.gather_rows(global_emb, idx, normalize=True, unique=True))
        return loss

    def get_l2_reg(self, users, pos_items, neg_items):
        self._check_ids((users, self.num_users), (pos_items, self.num_items), (neg_items, self.num_items))
        return self._l2_reg(users, pos_items, neg_items)

    def _l2_reg(self, users, pos_items, neg_items):
        u = ops.gather_rows_sorted(self.embedding_user.weight, users)
        i = ops.gather_rows_sorted(self.embedding_item.weight, torch.cat([pos_items, neg_items]))
        return 0.5 * (u.pow(2).sum() + i.pow(2).sum())

    def train_step(self, users, pos_items, neg_items, optimizer):
        """One step of the reference loop (:265-289) in fp32 on the row-restricted path: the local view
        is propagated once and only the batch's rows are read from it, the SVD view is formed for the SSL
        rows only. pos_items / neg_items are item ids (0-based, as the dataset yields them). Returns
        (bpr, ssl, reg) as detached device scalars."""
        nu, b = self.num_users, users.numel()
        self._check_ids((users, nu), (pos_items, self.num_items), (neg_items, self.num_items))
        optimizer.zero_grad()
        all_emb = self.all_embeddings()
        local = ops.lightgcl_propagate(all_emb, self.adj, self.n_layers)
        uu = torch.unique(users)
        ui = torch.unique(pos_items) + nu
        rows = ops.gather_rows_sorted(local, torch.cat([users, pos_items + nu, neg_items + nu, uu, ui]))
        bpr_loss = self._bpr(rows[:b], rows[b:2 * b], rows[2 * b:3 * b])
        glob = ops.lightgcl_global_rows(all_emb, self.view, torch.cat([uu, ui]), self.n_layers)
        k = uu.numel()
        ssl_rows, glob = ops.l2_normalize(rows[3 * b:]), ops.l2_normalize(glob)
        ssl_loss = self._info_nce(ssl_rows[:k], glob[:k]) + self._info_nce(ssl_rows[k:], glob[k:])
        reg_loss = self._l2_reg(users, pos_items, neg_items)
        loss = bpr_loss + self.lambda_ssl * ssl_loss + self.lambda_reg * reg_loss
        loss.backward()
        optimizer.step()
        return bpr_loss.detach(), ssl_loss.detach(), reg_loss.detach()
