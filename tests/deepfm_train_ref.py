"""CPU reference of one DeepFM training step (helper of test_gpu_deepfm_train.py and
test_deepfm_train_cpu.py; no tests here): oracle.deepfm.deepfm_forward with the tables as autograd
leaves, F.binary_cross_entropy_with_logits, torch.autograd.grad, per-field sparse gradients over
the batch's distinct ids, torch.optim.SparseAdam on the tables and torch.optim.Adam on the dense
parameters. float64 by default; float32 for the self-check of the end-to-end cap."""
import torch
import torch.nn.functional as F

from oracle import deepfm as OD

DENSE = ("w1", "b1", "w2", "b2", "wo", "bias")


def make_params(vocabs, seed=0, init_std=0.05):
    """float32 CPU parameters with every term alive: std 0.05 everywhere, non-zero biases."""
    g = torch.Generator().manual_seed(seed)
    nf = len(vocabs)

    def rn(*shape):
        return torch.randn(*shape, generator=g) * init_std

    return {"emb": [rn(v, 16) for v in vocabs], "lin": [rn(v, 1) for v in vocabs],
            "w1": rn(256, nf * 16), "b1": rn(256), "w2": rn(128, 256), "b2": rn(128), "wo": rn(1, 128),
            "bias": rn(1)}


def zipf_ids(R, vocabs, gen, a=1.1):
    """[R, F] int64 ids, field f ~ Zipf(a) over its vocab; the hot id differs per field."""
    cols = []
    for f, v in enumerate(vocabs):
        p = 1.0 / torch.arange(1, v + 1, dtype=torch.float64) ** a
        ids = torch.multinomial(p, R, replacement=True, generator=gen)
        cols.append((ids + 7 * f) % v)
    return torch.stack(cols, dim=1)


def labels(R, gen):
    return (torch.rand(R, generator=gen) < 0.4).float()


def gradients(params, x, y, reduction="mean", dtype=torch.float64, drop=()):
    """-> (loss, logit, dense gradients {name: tensor}, per field (distinct ids, dV [U,16], dW [U])).
    drop: (row, field) pairs whose gradient contribution is left out; the pair's forward still reads
    the row x names (realised by a duplicate of that row appended to the field's table)."""
    emb = [t.to(dtype) for t in params["emb"]]
    lin = [t.to(dtype) for t in params["lin"]]
    x = x.clone()
    for r, f in drop:
        i = int(x[r, f])
        emb[f] = torch.cat([emb[f], emb[f][i:i + 1]])
        lin[f] = torch.cat([lin[f], lin[f][i:i + 1]])
        x[r, f] = emb[f].shape[0] - 1
    emb = [t.clone().requires_grad_() for t in emb]
    lin = [t.clone().requires_grad_() for t in lin]
    dense = {k: params[k].to(dtype).clone().requires_grad_() for k in DENSE}
    logit, _ = OD.deepfm_forward(x, emb, lin, dense["bias"], [dense["w1"], dense["w2"]], [dense["b1"], dense["b2"]],
                                 dense["wo"], dtype=dtype)
    loss = F.binary_cross_entropy_with_logits(logit, y.to(dtype), reduction=reduction)
    leaves = emb + lin + [dense[k] for k in DENSE]
    gs = torch.autograd.grad(loss, leaves)
    nf = len(emb)
    sparse = []
    for f in range(nf):
        vocab = params["emb"][f].shape[0]
        ids = torch.unique(x[:, f])
        ids = ids[ids < vocab]
        sparse.append((ids, gs[f][ids], gs[nf + f][ids].reshape(-1)))
    return loss.detach(), logit.detach(), dict(zip(DENSE, gs[2 * nf:])), sparse


class RefTrainer:
    """SparseAdam on the tables + Adam on the dense parameters, one shared step count."""

    def __init__(self, params, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, reduction="mean", dtype=torch.float64):
        self.dtype, self.reduction = dtype, reduction
        self.p = {"emb": [t.to(dtype).clone() for t in params["emb"]], "lin": [t.to(dtype).clone() for t in params["lin"]]}
        for k in DENSE:
            self.p[k] = params[k].to(dtype).clone()
        self.tables = self.p["emb"] + self.p["lin"]
        self.sparse_opt = torch.optim.SparseAdam(self.tables, lr=lr, betas=betas, eps=eps)
        self.dense_opt = torch.optim.Adam([self.p[k] for k in DENSE], lr=lr, betas=betas, eps=eps)

    def seed_moments(self, m, v, step):
        """exp_avg / exp_avg_sq of every table (emb then lin order) and the step count so far."""
        for t, mi, vi in zip(self.tables, m, v):
            self.sparse_opt.state[t] = {"step": step, "exp_avg": mi.to(self.dtype).reshape(t.shape).clone(),
                                        "exp_avg_sq": vi.to(self.dtype).reshape(t.shape).clone()}

    def moments(self):
        st = self.sparse_opt.state
        return [st[t]["exp_avg"] for t in self.tables], [st[t]["exp_avg_sq"] for t in self.tables]

    def apply_sparse(self, sparse):
        """SparseAdam step from per-field (ids, dV [U,16], dW [U])."""
        nf = len(self.p["emb"])
        for f, (ids, dv, dw) in enumerate(sparse):
            for t, val in ((self.tables[f], dv), (self.tables[nf + f], dw.reshape(-1, 1))):
                t.grad = torch.sparse_coo_tensor(ids[None], val.to(self.dtype), t.shape)
        self.sparse_opt.step()

    def step(self, x, y, drop=(), max_grad_norm=None):
        loss, _, dense, sparse = gradients(self.p, x, y, self.reduction, self.dtype, drop)
        self.apply_sparse(sparse)
        for k in DENSE:
            self.p[k].grad = dense[k]
        if max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_([self.p[k] for k in DENSE], max_grad_norm)
        self.dense_opt.step()
        return loss


def cap_violations(a, b, lr):
    """(fraction of elements with |a - b| > 1e-2 lr, max |a - b| / lr): the end-to-end condition
    is fraction <= 1e-3 and max <= 3."""
    d = (a.double() - b.double()).abs() / lr
    return float((d > 1e-2).double().mean()), float(d.max())


def all_tensors(p):
    """(name, tensor) over every parameter of a params dict."""
    out = [(f"emb{f}", t) for f, t in enumerate(p["emb"])] + [(f"lin{f}", t) for f, t in enumerate(p["lin"])]
    return out + [(k, p[k]) for k in DENSE]
