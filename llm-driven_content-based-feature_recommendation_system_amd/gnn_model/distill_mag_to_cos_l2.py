"""Drop-in for gnn_model/distill_mag_to_cos_l2.py: distil LightGCL's dot-product scores into unit
vectors, so that a trained LightGCL can feed the cosine retrieval path (ops.retrieve_topk, the
similarity route, a FAISS / pgvector index) with its popularity signal intact.

Reference (gnn_model/distill_mag_to_cos_l2.py): MagnitudeEncoder :6-35, train_projector :40-105, the
commented projection of both tables :112-126.
Compute: one training step is two launches (ops.distill_step: rsx_distill_grads gathers the pairs'
rows, runs the forward, the MSE and the backward into per-workgroup slots; rsx_distill_apply adds the
slots in slot order and applies Adam), fp32 products, no float atomics, bit-reproducible. The eval
forward over a whole table is one kernel (ops.magnitude_encode). There is no CPU path for the trainer;
MagnitudeEncoder.forward itself falls back to its own torch sub-modules wherever the kernel does not
apply (CPU tensors, other widths, autograd recording, active dropout).
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from .. import ops


class MagnitudeEncoder(nn.Module):
    """Linear(input_dim, hidden_dim) + LeakyReLU(0.2) + Dropout(0.1) + Linear(hidden_dim, output_dim),
    the output L2-normalised, and the learnable logit_scale = log(1 / 0.07) that stretches cosines to
    the teacher's score range (:6-35; the same module tree, so the same state_dict and, under one
    seed, the same initial weights)."""

    def __init__(self, input_dim=64, output_dim=64, hidden_dim=128):
        super().__init__()
        self.encoder = nn.Sequential(
            nn.Linear(input_dim, hidden_dim),
            nn.LeakyReLU(0.2),
            nn.Dropout(0.1),
            nn.Linear(hidden_dim, output_dim),
        )
        self.logit_scale = nn.Parameter(torch.ones([]) * math.log(1 / 0.07))

    @property
    def widths(self):
        return self.encoder[0].in_features, self.encoder[0].out_features, self.encoder[3].out_features

    def dropout_p(self):
        """The hidden layer's dropout probability as it acts now: 0 in eval mode."""
        return float(self.encoder[2].p) if self.training else 0.0

    def _kernel_applies(self, x):
        """The forward kernel serves fp32 ROCm rows of the widths (64, 128, 64) when dropout is inactive
        (eval mode, or p == 0) and autograd is not recording (grad mode off, or neither x nor a
        parameter requires a gradient)."""
        return (self.dropout_p() == 0.0 and not (torch.is_grad_enabled() and (
                    x.requires_grad or any(p.requires_grad for p in self.parameters())))
                and x.is_cuda and x.dtype == torch.float32 and x.dim() == 2
                and ops.distill_supported(*self.widths) is None)

    def forward(self, x):
        if self._kernel_applies(x):
            lin1, act, _, lin2 = self.encoder
            return ops.magnitude_encode(x, lin1.weight, lin1.bias, lin2.weight, lin2.bias, slope=act.negative_slope)
        return F.normalize(self.encoder(x), p=2, dim=1)

    def make_trainer(self, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        return DistillTrainer(self, lr, betas, eps)


class DistillTrainer:
    """torch.optim.Adam(projector.parameters(), lr) fused into the distillation step (:48, :96-98):
    owns the flat moments exp_avg / exp_avg_sq [16,577] (parameter order) and the step count."""

    def __init__(self, module, lr=1e-3, betas=(0.9, 0.999), eps=1e-8):
        why = ops.distill_supported(*module.widths)
        if why:
            raise NotImplementedError(f"DistillTrainer: {why}")
        self.module, self.lr, self.betas, self.eps = module, float(lr), (float(betas[0]), float(betas[1])), float(eps)
        self.steps = 0
        self.exp_avg = self.exp_avg_sq = self.flag = None
        self.guard = ops.IdRangeGuard("distillation pairs (embedding_user / embedding_item rows)")

    def _state(self, device):
        if self.exp_avg is None or self.exp_avg.device != device:
            if self.steps:
                raise RuntimeError("DistillTrainer: the module moved to another device between steps")
            self.exp_avg = torch.zeros(ops.DISTILL_PARAMS, device=device, dtype=torch.float32)
            self.exp_avg_sq = torch.zeros_like(self.exp_avg)
            self.flag = torch.zeros(1, device=device, dtype=torch.int32)

    def step(self, user_table, item_table, users, items, seed=None):
        """One fused step on the pairs (users[k], items[k]): the module's five parameters updated in
        place, the loss returned as a 0-d float64 device tensor; no host read. Dropout (the module's p)
        acts only in train() mode; seed None draws ops.next_seed() then."""
        m = self.module
        lin1, act, _, lin2 = m.encoder
        p = m.dropout_p()
        if seed is None:
            seed = ops.next_seed() if p > 0 else 0
        self._state(lin1.weight.device)
        out = ops.distill_step(user_table, item_table, users, items, lin1.weight, lin1.bias, lin2.weight, lin2.bias,
                               m.logit_scale, slope=act.negative_slope, p_drop=p, seed=seed, update=True,
                               exp_avg=self.exp_avg, exp_avg_sq=self.exp_avg_sq, step=self.steps + 1, lr=self.lr,
                               betas=self.betas, adam_eps=self.eps, flag=self.flag)
        self.steps += 1
        return out.loss

    def check(self):
        """Raise IndexError if any step so far met an id outside its table (one host read; such a pair
        contributed nothing to its step)."""
        if self.flag is None:
            return
        self.guard.watch(self.flag)
        try:
            self.guard.check()
        except IndexError:
            self.flag.zero_()
            raise


class edge_batches:
    """(users, pos_items, None) batches over every edge of a TrainDataset once per iteration, cut from
    its users / items tensors on their device (a fresh permutation per iteration when shuffle, drawn
    from generator on the generator's device; the last batch is short). Re-iterable, so it serves
    train_projector as the dataloader of every epoch. The distillation ignores the negative item, so
    none is sampled and no edge goes through __getitem__."""

    def __init__(self, dataset, batch_size, generator=None, shuffle=True):
        if int(batch_size) < 1:
            raise ValueError(f"edge_batches: batch_size must be at least 1 (got {batch_size})")
        self.dataset, self.batch_size, self.generator, self.shuffle = dataset, int(batch_size), generator, shuffle

    def __len__(self):
        return (self.dataset.users.numel() + self.batch_size - 1) // self.batch_size

    def __iter__(self):
        users, items = self.dataset.users, self.dataset.items
        n = users.numel()
        if self.shuffle:
            gen = self.generator
            perm = torch.randperm(n, generator=gen, device=gen.device if gen is not None else users.device)
            perm = perm.to(users.device)
            users, items = users[perm], items[perm]
        for o in range(0, n, self.batch_size):
            yield users[o:o + self.batch_size].long(), items[o:o + self.batch_size].long(), None


def train_projector(lightgcl_model, dataloader, device, epochs=5, lr=0.001, log=print):
    """Distil the teacher's scores <u, i> on the training edges into a MagnitudeEncoder whose
    cos(student_u, student_i) exp(logit_scale) reproduces them (MSE, Adam; :40-105). Teacher rows are
    the raw embedding_user / embedding_item tables, as in the reference. dataloader: any iterable of
    (users, pos_items, _) batches, iterated once per epoch (a DataLoader, edge_batches, a list). The
    loss is accumulated on the device: one host read per
    epoch, where an out-of-range id also raises its IndexError. Returns the projector."""
    lightgcl_model.eval()
    projector = MagnitudeEncoder(input_dim=64, output_dim=64).to(device)
    trainer = projector.make_trainer(lr=lr)
    src_user_emb = lightgcl_model.embedding_user.weight.detach()
    src_item_emb = lightgcl_model.embedding_item.weight.detach()
    log("Start Projector Distillation...")
    for epoch in range(epochs):
        projector.train()
        total, steps = torch.zeros((), device=device, dtype=torch.float64), 0
        for batch_users, batch_pos_items, _ in dataloader:
            total += trainer.step(src_user_emb, src_item_emb, batch_users.to(device), batch_pos_items.to(device))
            steps += 1
        mean = float(total) / max(steps, 1)
        trainer.check()
        log(f"Epoch {epoch + 1}/{epochs} | Distillation Loss: {mean:.4f}")
    return projector


def project_tables(projector, lightgcl_model):
    """(user_unit, item_unit): both raw tables through the projector in eval mode (:112-126), unit rows
    that carry the popularity signal in their angles."""
    was_training = projector.training
    projector.eval()
    try:
        with torch.no_grad():
            return (projector(lightgcl_model.embedding_user.weight.detach()),
                    projector(lightgcl_model.embedding_item.weight.detach()))
    finally:
        projector.train(was_training)
