"""Float64 torch restatement of one training step of the DCN-V2 RankingModel -- TEST INFRASTRUCTURE ONLY.

Forward as oracle/ranker.py (its crossnet is imported), with an optional given dropout mask after
the first LayerNorm + GELU; binary_cross_entropy_with_logits; gradients by autograd;
torch.optim.AdamW. Parameters travel as a dict under the RankingModel's state_dict names
(cross_net.kernels.l [D, 1], cross_net.biases.l [D], deep_net.{0,1,4,5}.{weight,bias},
final_head.{weight,bias}). `crossnet_bwd` is the closed-form backward of the cross network that
rsx_crossnet_bwd implements; it runs in the dtype of its inputs, so the same text serves as the
float64 reference and as the plain fp32 restatement.
"""
import torch
import torch.nn.functional as F

from oracle import ranker as OR


def n_layers(sd):
    return sum(1 for k in sd if k.startswith("cross_net.kernels."))


def param_names(sd):
    """The trainer's parameter order: kernels, biases, both linears with their LayerNorms, final_head."""
    L = n_layers(sd)
    return ([f"cross_net.kernels.{l}" for l in range(L)] + [f"cross_net.biases.{l}" for l in range(L)]
            + [f"deep_net.{i}.{n}" for i in (0, 1, 4, 5) for n in ("weight", "bias")]
            + ["final_head.weight", "final_head.bias"])


def cross_head(x, ks, bs, wh):
    """(x_L, head_part) of the cross network in x's dtype (tests/test_gpu_glue.py's restatement)."""
    x0, xl = x, x
    for k, b in zip(ks, bs):
        xl = x0 * ((xl * k.reshape(-1)).sum(-1, keepdim=True) + b) + xl
    return xl, (xl * wh).sum(-1) if wh is not None else None


def crossnet_bwd(x, ks, bs, w_head=None, dhead=None, dx_out=None):
    """Closed form. x [B, D], ks / bs: L tensors of D elements, upstream dhead [B] (gradient of
    <x_L, w_head>) and / or dx_out [B, D] (gradient of x_L) -> (dk list [D], db list [D], dw_head [D]
    or None, dx [B, D]). Per row, G = dx_{l+1}, l going down: db_l += G x_0; ds = <G, x_0>;
    dk_l += ds x_l; dx_0 += G (s_l + b_l); G += ds k_l; dx = dx_0 + G."""
    ks = [k.reshape(-1) for k in ks]
    L = len(ks)
    xs, ss = [x], []
    for k, b in zip(ks, bs):
        s = (xs[-1] * k).sum(-1, keepdim=True)
        ss.append(s)
        xs.append(x * (s + b) + xs[-1])
    G = torch.zeros_like(x)
    dwh = None
    if dhead is not None:
        G = G + dhead.reshape(-1, 1) * w_head
        dwh = (dhead.reshape(-1, 1) * xs[L]).sum(0)
    if dx_out is not None:
        G = G + dx_out
    dx0 = torch.zeros_like(x)
    dk, db = [None] * L, [None] * L
    for l in range(L - 1, -1, -1):
        db[l] = (G * x).sum(0)
        ds = (G * x).sum(-1, keepdim=True)
        dk[l] = (ds * xs[l]).sum(0)
        dx0 = dx0 + G * (ss[l] + bs[l])
        G = G + ds * ks[l]
    return dk, db, dwh, dx0 + G


def forward(sd, x, mask=None, p=0.0):
    """Logits [B] in float64 (and the post-dropout h1, x_L). mask: the [B, 256] keep-mask (bool) of the
    dropout after the first GELU, kept elements scaled by 1 / (1 - p); None: no dropout."""
    sd = {k: v.double() for k, v in sd.items()}
    x = x.double()
    L = n_layers(sd)
    cross = OR.crossnet(x, [sd[f"cross_net.kernels.{l}"] for l in range(L)],
                        [sd[f"cross_net.biases.{l}"] for l in range(L)])
    h1 = F.gelu(F.layer_norm(F.linear(x, sd["deep_net.0.weight"], sd["deep_net.0.bias"]), (256,),
                             sd["deep_net.1.weight"], sd["deep_net.1.bias"], 1e-5))
    if mask is not None:
        h1 = h1 * mask.double() / (1.0 - p)
    h2 = F.gelu(F.layer_norm(F.linear(h1, sd["deep_net.4.weight"], sd["deep_net.4.bias"]), (128,),
                             sd["deep_net.5.weight"], sd["deep_net.5.bias"], 1e-5))
    logits = F.linear(torch.cat([cross, h2], 1), sd["final_head.weight"], sd["final_head.bias"]).squeeze(1)
    return logits, h1, cross


def step_grads(sd, x, y, reduction="mean", mask=None, p=0.0):
    """(loss, logits, {name: gradient}) of one step in float64 by autograd."""
    leaves = {k: v.detach().double().clone().requires_grad_() for k, v in sd.items()}
    logits, _, _ = forward(leaves, x, mask, p)
    loss = F.binary_cross_entropy_with_logits(logits, y.double(), reduction=reduction)
    names = param_names(sd)
    grads = torch.autograd.grad(loss, [leaves[n] for n in names])
    return loss.detach(), logits.detach(), dict(zip(names, grads))


def train(sd, batches, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, reduction="mean",
          max_grad_norm=None, masks=None, p=0.0):
    """AdamW steps in float64 over batches [(x, y), ...] (masks: one per batch or None) -> (the
    parameters after the last step, the losses)."""
    names = param_names(sd)
    params = {n: sd[n].detach().double().clone().requires_grad_() for n in names}
    opt = torch.optim.AdamW([params[n] for n in names], lr=lr, betas=betas, eps=eps, weight_decay=weight_decay)
    losses = []
    for i, (x, y) in enumerate(batches):
        opt.zero_grad()
        logits, _, _ = forward(params, x, None if masks is None else masks[i], p)
        loss = F.binary_cross_entropy_with_logits(logits, y.double(), reduction=reduction)
        loss.backward()
        if max_grad_norm is not None:
            torch.nn.utils.clip_grad_norm_([params[n] for n in names], max_grad_norm)
        opt.step()
        losses.append(loss.detach())
    return {n: v.detach() for n, v in params.items()}, losses
