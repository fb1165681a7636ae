"""Adversarial patch: a small image patch optimised through the encoder, the RSSM posterior and the imagination.

The patch is pasted into every frame of a batch (csrc/attack.hip: sd_patch_apply), the world model's posterior of the
patched frames is compared with the posterior of the clean frames (PosteriorAttackLoss) and, with `w_return`, rolled
out by the frozen actor to its imagined lambda-return (PlanningAttackLoss: Dreamer.imagined_return, whose backward is
ops.ImagineReturnFn). The loss is differentiated to the image (Dreamer.posterior(with_grad=True): the first encoder
stage's input gradient is sd_conv2d_dgrad_pool), folded back onto the patch (sd_patch_grad) and one Adam step +
projection is taken (sd_patch_step). DESIGN.md §4.4c.

    from sdreamer.attack import load_attack_config, train_patch
    patch, log = train_patch(agent, [(data, initial), ...], load_attack_config(["steps=200", "w_action=1.0"]))
    patch, log = train_patch(agent, batches, load_attack_config(["w_return=1.0", "w_kl=0.0"]))  # upstream's default
"""
from __future__ import annotations

import torch

from . import kernels as K
from . import ops
from .config import load_config

PLACEMENTS = ("bottom_center", "top_center", "center", "fixed", "saliency")
LOG_KEYS = ("loss", "kl", "action", "tv")
LOG_KEYS_PLANNING = LOG_KEYS + ("ret",)  # the log's columns with w_return != 0
SALIENCY_SIGMA = 0.05  # the seeded image perturbation at which the saliency gradient is taken


def load_attack_config(overrides=None, name="attack/adv_patch"):
    """configs/attack/adv_patch.yaml with `k=v` overrides (as config.load_config)."""
    return load_config(name, overrides)


# ------------------------------------------------------------------------------------------------- placement
def placement_offset(placement, image_hw, patch_hw, x0=0, y0=0):
    """(row, column) of the patch's top-left corner. `fixed` takes (y0, x0) as given (it may leave the image: the
    window is clipped); `saliency` is resolved from a gradient (saliency_offset) and has no closed form."""
    (H, W), (ph, pw) = image_hw, patch_hw
    if placement == "bottom_center":
        return H - ph, (W - pw) // 2
    if placement == "top_center":
        return 0, (W - pw) // 2
    if placement == "center":
        return (H - ph) // 2, (W - pw) // 2
    if placement == "fixed":
        return int(y0), int(x0)
    if placement == "saliency":
        raise ValueError("saliency placement is resolved from a gradient: saliency_offset(|d_image|, patch_hw)")
    raise ValueError(f"placement {placement!r} not in {PLACEMENTS}")


def clipped_window(offset, image_hw, patch_hw):
    """The part of the patch window that lies in the image: ((y_lo, y_hi, x_lo, x_hi) in image coordinates,
    (py_lo, px_lo) the patch element at its first pixel); y_hi <= y_lo or x_hi <= x_lo: nothing lands."""
    (oy, ox), (H, W), (ph, pw) = offset, image_hw, patch_hw
    y_lo, y_hi = min(max(oy, 0), H), max(min(oy + ph, H), 0)
    x_lo, x_hi = min(max(ox, 0), W), max(min(ox + pw, W), 0)
    return (y_lo, max(y_hi, y_lo), x_lo, max(x_hi, x_lo)), (y_lo - oy, x_lo - ox)


def saliency_offset(saliency, patch_hw):
    """The top-left corner of the patch_hw window with the largest sum of `saliency` (H, W) (non-negative; the first
    such window in row-major order)."""
    ph, pw = patch_hw
    H, W = saliency.shape
    if ph > H or pw > W:
        raise ValueError("the patch does not fit the image")
    c = torch.zeros(H + 1, W + 1, dtype=torch.float64, device=saliency.device)
    c[1:, 1:] = saliency.double().cumsum(0).cumsum(1)
    win = c[ph:, pw:] - c[:-ph, pw:] - c[ph:, :-pw] + c[:-ph, :-pw]
    i = int(win.argmax())
    return i // win.shape[1], i % win.shape[1]


def eot_offsets(base, n, copies, generator, max_jitter):
    """(n * (1 + copies), 2) int32 offsets: the first n rows are `base`, every further copy of the batch adds a
    per-image jitter in [-max_jitter, max_jitter]^2 drawn from `generator` (a seeded CPU torch.Generator)."""
    out = torch.tensor(base, dtype=torch.int32).repeat(n * (1 + copies), 1)
    if copies:
        out[n:] += torch.randint(-max_jitter, max_jitter + 1, (n * copies, 2), generator=generator, dtype=torch.int32)
    return out


# ------------------------------------------------------------------------------------------------- the patch
class AdversarialPatch:
    """The patch (ph, pw, C) f32 in [0, 1] with its Adam state on the device.

    placement: bottom_center | top_center | center | fixed (x0, y0) | saliency (set by train_patch from the first
    batch; until then the center). eps: L-inf radius around the initial patch (None: any value in [0, 1]).
    eot_translations: extra copies of the batch per step, each image with its own offset jitter (seeded)."""

    def __init__(self, image_hw=(64, 64), channels=3, patch_hw=(16, 16), placement="bottom_center", x0=0, y0=0,
                 eps=None, eot_translations=0, lr=0.05, max_jitter=4, seed=0, device="cuda", init=0.5):
        if placement not in PLACEMENTS:
            raise ValueError(f"placement {placement!r} not in {PLACEMENTS}")
        self.image_hw, self.patch_hw = tuple(int(v) for v in image_hw), tuple(int(v) for v in patch_hw)
        self.placement, self.x0, self.y0 = placement, int(x0), int(y0)
        self.eps = None if eps is None else float(eps)
        self.eot_translations, self.max_jitter, self.lr = int(eot_translations), int(max_jitter), float(lr)
        self.generator = torch.Generator().manual_seed(int(seed))
        shape = (*self.patch_hw, int(channels))
        self.patch = (init.to(device=device, dtype=torch.float32).reshape(shape).clone() if torch.is_tensor(init)
                      else torch.full(shape, float(init), dtype=torch.float32, device=device))
        self.base = self.patch.clone() if self.eps is not None else None
        self.m, self.v = torch.zeros_like(self.patch), torch.zeros_like(self.patch)
        self.steps = torch.zeros(1, dtype=torch.int32, device=device)
        self.offset = placement_offset("center" if placement == "saliency" else placement, self.image_hw,
                                       self.patch_hw, x0, y0)

    def offsets(self, n, jitter=True):
        """(n * (1 + eot_translations), 2) int32 device offsets for a batch of n images (see eot_offsets)"""
        copies = self.eot_translations if jitter else 0
        return eot_offsets(self.offset, n, copies, self.generator, self.max_jitter).to(self.patch.device)

    def apply(self, images, offsets, need_f32=True):
        """images (..., H, W, C) uint8 or f32 in [0, 1], offsets (N, 2) for the N = prod(...) images -> (composited
        f32 images or None, the encoder input: - 0.5, channel-padded), both with the leading shape of `images`."""
        lead = images.shape[:-3]
        f, enc = K.patch_apply(images.reshape(-1, *images.shape[-3:]).contiguous(), self.patch, offsets,
                               need_f32=need_f32)
        return (None if f is None else f.view(*lead, *f.shape[-3:])), enc.view(*lead, *enc.shape[-3:])

    def grad(self, d_image, offsets, w_tv=0.0):
        """(d_patch, tv): the image gradient folded onto the patch (+ w_tv * d TV / d patch), and the patch's TV"""
        return K.patch_grad(d_image.reshape(-1, *d_image.shape[-3:]).contiguous(), offsets, self.patch_hw,
                            patch=self.patch, w_tv=w_tv)

    def step(self, d_patch):
        """one Adam step on the patch, then the projections onto [0, 1] and the eps ball (one launch)"""
        K.patch_step(self.patch, d_patch, self.m, self.v, self.steps, self.lr, base=self.base, eps=self.eps)
        return self.patch


# ------------------------------------------------------------------------------------------------- the objective
class PosteriorAttackLoss:
    """loss = -(w_kl * KL + w_action * shift): minimising it maximises the posterior's and the policy's shift.

    KL: the categorical KL(clean posterior || patched posterior) summed over the latents (rssm.kl_loss's kernels,
    no free bits), mean over B and T; the clean posterior is detached. shift: the mean squared difference of the
    actor's mode on the patched and the clean posterior features (tanh mean for continuous actions, the unimix
    probabilities for discrete ones), the actor run with a gradient to its input. w_tv weighs the patch's anisotropic
    total variation, which the patch-gradient kernel adds (AdversarialPatch.grad); it does not enter __call__."""

    def __init__(self, w_kl=1.0, w_action=0.0, w_tv=0.01, w_return=0.0):
        if float(w_return) != 0.0:
            raise NotImplementedError(
                "w_return: the imagined-return term needs a backward through the imagination rollout, and the fused "
                "imagination kernels (sd_imagine) are forward-only (no_grad by design): PlanningAttackLoss has that "
                "term (Dreamer.imagined_return); see DESIGN.md §4.4c")
        self.w_kl, self.w_action, self.w_tv = float(w_kl), float(w_action), float(w_tv)

    def actor_mode(self, agent, post_stoch, post_deter):
        feat = agent.rssm.get_feat(post_stoch, post_deter)
        logits = agent.actor(feat.reshape(-1, feat.shape[-1]))
        if agent.act_discrete:
            u = float(agent.config.actor.dist.unimix_ratio)
            return torch.softmax(logits, -1) * (1.0 - u) + u / logits.shape[-1]
        return torch.tanh(logits[:, :agent.act_dim])

    @torch.no_grad()
    def clean(self, agent, post):
        """the detached clean side: (clean posterior logits, clean actor mode or None)"""
        post_stoch, post_deter, post_logit = (t.detach() for t in post)
        mode = self.actor_mode(agent, post_stoch, post_deter) if self.w_action else None
        return post_logit, mode

    def __call__(self, agent, clean, post_stoch, post_deter, post_logit):
        """-> (loss, {"kl": ..., "action": ...}) as 0-dim device tensors"""
        clean_logit, clean_mode = clean
        zero = torch.zeros((), dtype=torch.float32, device=post_logit.device)
        kl = act = zero
        if self.w_kl:
            dyn, _ = agent.rssm.kl_loss(clean_logit, post_logit, 0.0)  # d KL(clean || patched) / d patched
            kl = dyn.mean()
        if self.w_action:
            act = ((self.actor_mode(agent, post_stoch, post_deter) - clean_mode) ** 2).mean()
        return -(self.w_kl * kl + self.w_action * act), {"kl": kl.detach(), "action": act.detach()}


class PlanningAttackLoss:
    """loss = w_return * mean(ret0) - (w_kl * KL + w_action * shift): minimising it lowers the agent's imagined
    return. ret0 (B * T,): Dreamer.imagined_return from every patched posterior state, `horizon` steps (None: the
    agent's imag_horizon), the imagination's noise from the batch's seed. KL, shift and clean() are
    PosteriorAttackLoss's; w_tv as there."""

    def __init__(self, w_return=1.0, w_kl=0.0, w_action=0.0, w_tv=0.01, horizon=None):
        self.posterior = PosteriorAttackLoss(w_kl, w_action, w_tv)
        self.w_return, self.w_kl, self.w_action, self.w_tv = float(w_return), float(w_kl), float(w_action), float(w_tv)
        self.horizon = None if horizon is None else int(horizon)

    def clean(self, agent, post):
        return self.posterior.clean(agent, post)

    def __call__(self, agent, clean, post_stoch, post_deter, post_logit, seed=0):
        """-> (loss, {"kl": ..., "action": ..., "ret": mean(ret0)}) as 0-dim device tensors"""
        total, terms = self.posterior(agent, clean, post_stoch, post_deter, post_logit)
        if self.w_return:
            ret = agent.imagined_return(post_stoch, post_deter, self.horizon, seed=seed).mean()
            total = self.w_return * ret + total
        else:
            ret = torch.zeros((), dtype=torch.float32, device=post_logit.device)
        terms["ret"] = ret.detach()
        return total, terms


def make_loss(cfg):
    """The objective a configuration asks for: PlanningAttackLoss with w_return != 0, else PosteriorAttackLoss"""
    w_return = float(cfg.get("w_return", 0.0))
    if w_return != 0.0:
        return PlanningAttackLoss(w_return, cfg.w_kl, cfg.w_action, cfg.w_tv, cfg.get("horizon", None))
    return PosteriorAttackLoss(cfg.w_kl, cfg.w_action, cfg.w_tv, w_return)


def _evaluate(loss, agent, clean, post, seed):
    if isinstance(loss, PlanningAttackLoss):
        return loss(agent, clean, *post, seed=seed)
    return loss(agent, clean, *post)


# ------------------------------------------------------------------------------------------------- the loop
def _tile(t, copies):
    return t if copies == 0 else t.repeat(1 + copies, *([1] * (t.dim() - 1)))


def _f32_image(img):
    return K.u8_to_f32(img.contiguous()) if img.dtype == torch.uint8 else img


def attack_gradient(agent, patch, loss, data, initial, seed, offsets, clean=None):
    """One evaluation of the objective on a batch with the patch at `offsets` (N * copies rows: the batch is tiled to
    match, and a PlanningAttackLoss imagines from the tiled rows): -> (loss, terms, d_image, clean). No parameter
    gradient is written (ops.grad_sink_scope)."""
    B, T = data["action"].shape[:2]
    copies = offsets.shape[0] // (B * T) - 1
    tiled = {k: _tile(v, copies) for k, v in data.items() if k != "__enc_image"}
    init = tuple(_tile(t, copies) for t in initial)
    if clean is None:
        clean = loss.clean(agent, agent.posterior(tiled, init, seed=seed))
    img, _ = patch.apply(tiled["image"], offsets)
    img.requires_grad_(True)
    with ops.grad_sink_scope():
        post = agent.posterior({**tiled, "image": img}, init, seed=seed, with_grad=True)
        total, terms = _evaluate(loss, agent, clean, post, seed)
        (d_image,) = torch.autograd.grad(total, img)
    return total.detach(), terms, d_image, clean


def _saliency(agent, loss, data, initial, seed, patch_hw, generator):
    """|d objective / d image| summed over the batch, time and channels, taken at a seeded perturbation of the clean
    frames (at the clean frames themselves the KL and action terms are stationary: their gradient is exactly zero;
    the return term's is not, but the perturbation stays so that the placement does not depend on the weights)."""
    img = _f32_image(data["image"])
    noise = torch.randn(img.shape, generator=generator).to(img.device)
    pert = (img + SALIENCY_SIGMA * noise).clamp_(0.0, 1.0).requires_grad_(True)
    clean = loss.clean(agent, agent.posterior(data, initial, seed=seed))
    with ops.grad_sink_scope():
        post = agent.posterior({**data, "image": pert}, initial, seed=seed, with_grad=True)
        total, _ = _evaluate(loss, agent, clean, post, seed)
        (g,) = torch.autograd.grad(total, pert)
    return saliency_offset(g.abs().sum(dim=(0, 1, 4)), patch_hw)


def train_patch(agent, batches, cfg, patch=None):
    """Optimise a patch against `agent` on `batches` (a list of (data, initial); data a dict of (B, T, *) device
    tensors, image uint8 or f32) for cfg.steps steps -> (patch (ph, pw, C), log (steps, 4)): the objective's terms
    per step in LOG_KEYS order (with cfg.w_return != 0: (steps, 5), LOG_KEYS_PLANNING, and the objective is
    PlanningAttackLoss), a device tensor (no host synchronisation in the loop). Step i uses batch i mod
    len(batches) with the posterior noise of seed cfg.seed + that batch's index; its clean posterior is computed
    once."""
    if agent.rep_loss == "dreamerpro":
        raise NotImplementedError("the patch attack with rep_loss=dreamerpro")
    if getattr(agent, "world", 1) > 1:
        raise NotImplementedError("the patch attack under data parallel")
    loss = make_loss(cfg)
    planning = isinstance(loss, PlanningAttackLoss)
    img0 = batches[0][0]["image"]
    B, T, H, W, C = img0.shape
    seed = int(cfg.get("seed", 0))
    if patch is None:
        patch = AdversarialPatch((H, W), C, tuple(cfg.patch_hw), cfg.placement, cfg.get("x0", 0), cfg.get("y0", 0),
                                 cfg.eps, cfg.eot_translations, cfg.lr, int(cfg.get("max_jitter", 4)), seed,
                                 device=img0.device)
    if patch.placement == "saliency":
        patch.offset = _saliency(agent, loss, *batches[0], seed, patch.patch_hw, patch.generator)
    steps = int(cfg.steps)
    log = torch.zeros(steps, len(LOG_KEYS_PLANNING if planning else LOG_KEYS), dtype=torch.float32,
                      device=img0.device)
    cleans = {}
    for i in range(steps):
        j = i % len(batches)
        data, initial = batches[j]
        offsets = patch.offsets(B * T)
        total, terms, d_image, cleans[j] = attack_gradient(agent, patch, loss, data, initial, seed + j, offsets,
                                                           cleans.get(j))
        d_patch, tv = patch.grad(d_image, offsets, loss.w_tv)
        log[i, 0], log[i, 1], log[i, 2], log[i, 3] = total + loss.w_tv * tv[0], terms["kl"], terms["action"], tv[0]
        if planning:
            log[i, 4] = terms["ret"]
        patch.step(d_patch)
    return patch.patch, log
