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

With eot_scale / eot_rotation / eot_contrast / eot_brightness the EoT copies are also scaled, rotated and re-lit: the
patch is then resampled bilinearly (sd_patch_apply_affine, its adjoint sd_patch_grad_affine) through per-image rows
built on the host (transform_rows). A trained patch is evaluated offline with evaluate_patch (clean against patched
imagined return, posterior KL, actor-mode shift per replay batch) and on the acting path with patched_act /
patched_policy_graph (Dreamer.act / Dreamer.policy_graph on composited observations).
"""
from __future__ import annotations

import math

import torch

from . import kernels as K
from . import ops
from .config import Config, load_config

PLACEMENTS = ("bottom_center", "top_center", "center", "fixed", "saliency")
LOG_KEYS = ("loss", "kl", "action", "tv")
LOG_KEYS_PLANNING = LOG_KEYS + ("ret",)  # the log's columns with w_return != 0
EVAL_KEYS = ("ret_clean", "ret_patched", "kl", "action")  # evaluate_patch's columns
SALIENCY_SIGMA = 0.05  # the seeded image perturbation at which the saliency gradient is taken
EOT_RANGE_KEYS = ("eot_scale", "eot_rotation", "eot_contrast", "eot_brightness")
TRANSFORM_SEED_OFFSET = 1_000_003  # AdversarialPatch's transform generator: manual_seed(seed + this)


def load_attack_config(overrides=None, name="attack/adv_patch"):
    """configs/attack/adv_patch.yaml with `k=v` overrides (as config.load_config)."""
    cfg = load_config(name, overrides)
    eot_ranges(cfg)
    return cfg


def eot_ranges(cfg, copies=None):
    """(scale (lo, hi), rotation_deg, contrast, brightness) of a configuration (missing keys: off). A range that is
    on while there are no EoT copies to act on (eot_translations: 0) is a ValueError naming the key."""
    scale = tuple(float(v) for v in cfg.get("eot_scale", (1.0, 1.0)))
    out = (scale, float(cfg.get("eot_rotation", 0.0)), float(cfg.get("eot_contrast", 0.0)),
           float(cfg.get("eot_brightness", 0.0)))
    _check_ranges(*out, int(cfg.get("eot_translations", 0)) if copies is None else copies)
    return out


def _check_ranges(scale, rotation_deg, contrast, brightness, copies):
    if len(scale) != 2 or not 0.0 < scale[0] <= scale[1]:
        raise ValueError(f"eot_scale {scale!r}: [lo, hi] with 0 < lo <= hi")
    if rotation_deg < 0.0 or contrast < 0.0 or brightness < 0.0:
        raise ValueError("eot_rotation, eot_contrast and eot_brightness are half-widths: >= 0")
    on = [k for k, v in zip(EOT_RANGE_KEYS, (scale != (1.0, 1.0), rotation_deg, contrast, brightness)) if v]
    if on and copies == 0:
        raise ValueError(f"{on[0]} acts on the extra copies of the batch that eot_translations makes: it needs "
                         f"eot_translations > 0 (max_jitter: 0 gives copies that vary only in {', '.join(on)})")
    return bool(on)


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


def transform_rows(offsets, params, patch_hw):
    """The kernels' transform rows (N, 8) f32 (sdhip.h: a00 a01 b0 a10 a11 b1 gain bias) of N images from their
    integer offsets (N, 2) and params (N, 4) = scale s, angle theta (radians), gain, bias; a host function, float64
    until the final rounding. A pixel centre (y, x) maps to the patch coordinates
        [u; v] = (1 / s) R(-theta) ([y; x] - c) + ((ph - 1) / 2, (pw - 1) / 2),  c = (oy + (ph - 1) / 2, ox + (pw - 1) / 2):
    the patch's centre stays where the offset puts it, the patch appears s times as large and turned by theta;
    s = 1, theta = 0 is the identity row of that offset (b = -offset). s <= 0 and non-finite values raise."""
    ph, pw = patch_hw
    off = torch.as_tensor(offsets).detach().cpu().to(torch.float64).reshape(-1, 2)
    par = torch.as_tensor(params).detach().cpu().to(torch.float64).reshape(-1, 4)
    if off.shape[0] != par.shape[0]:
        raise ValueError(f"transform_rows: {off.shape[0]} offsets for {par.shape[0]} parameter rows")
    s, th, gain, bias = par.unbind(1)
    if not bool(torch.isfinite(par).all()) or not bool(torch.isfinite(off).all()):
        raise ValueError("transform_rows: non-finite offset or parameter")
    if bool((s <= 0).any()):
        raise ValueError("transform_rows: the scale must be > 0")
    cos, sin = torch.cos(th) / s, torch.sin(th) / s
    a = torch.stack([cos, sin, -sin, cos], 1).view(-1, 2, 2)  # (1 / s) R(-theta)
    pc = torch.tensor([(ph - 1) / 2, (pw - 1) / 2], dtype=torch.float64)
    b = pc - torch.einsum("nij,nj->ni", a, off + pc)
    rows = torch.stack([a[:, 0, 0], a[:, 0, 1], b[:, 0], a[:, 1, 0], a[:, 1, 1], b[:, 1], gain, bias], 1)
    return check_rows((rows + 0.0).to(torch.float32))  # + 0.0: no negative zeros


def check_rows(rows):
    """refuses (ValueError) host rows (N, 8) with a non-finite entry or a singular 2 x 2; returns them"""
    r = rows.double()
    if not bool(torch.isfinite(r).all()):
        raise ValueError("transform rows: non-finite entry")
    if bool((r[:, 0] * r[:, 4] - r[:, 1] * r[:, 3] == 0).any()):
        raise ValueError("transform rows: singular 2 x 2")
    return rows


def eot_transforms(n, copies, generator, scale=(1.0, 1.0), rotation_deg=0.0, contrast=0.0, brightness=0.0):
    """(n * (1 + copies), 4) float64 parameters (scale, angle in radians, gain, bias; transform_rows' params): the
    first n rows are the identity (1, 0, 1, 0), the others come from one torch.rand((n * copies, 4), float64) of
    `generator`: scale in [scale[0], scale[1]], angle in +-rotation_deg pi / 180, gain in 1 +- contrast, bias in
    +-brightness."""
    out = torch.tensor([1.0, 0.0, 1.0, 0.0], dtype=torch.float64).repeat(n * (1 + copies), 1)
    if copies:
        r = torch.rand((n * copies, 4), generator=generator, dtype=torch.float64)
        out[n:, 0] = scale[0] + (scale[1] - scale[0]) * r[:, 0]
        out[n:, 1] = (2.0 * r[:, 1] - 1.0) * (rotation_deg * math.pi / 180.0)
        out[n:, 2] = 1.0 + (2.0 * r[:, 2] - 1.0) * contrast
        out[n:, 3] = (2.0 * r[:, 3] - 1.0) * brightness
    return out


# ------------------------------------------------------------------------------------------------- the patch
class AdversarialPatch:
    """The patch (ph, pw, C) f32 in [0, 1] with its Adam state on the device.

    placement: bottom_center | top_center | center | fixed (x0, y0) | saliency (set by train_patch from the first
    batch; until then the center). eps: L-inf radius around the initial patch (None: any value in [0, 1]).
    eot_translations: extra copies of the batch per step, each image with its own offset jitter (seeded).
    eot_scale (lo, hi), eot_rotation (degrees), eot_contrast, eot_brightness: each extra copy also gets its own
    scale, in-plane rotation, gain and bias (eot_transforms), drawn from a second seeded generator
    (seed + TRANSFORM_SEED_OFFSET) so that `generator`'s sequence (offsets, saliency noise) is what it is without
    them; all off (the default): transforms() is None and only the plain kernels are launched."""

    def __init__(self, image_hw=(64, 64), channels=3, patch_hw=(16, 16), placement="bottom_center", x0=0, y0=0,
                 eps=None, eot_translations=0, lr=0.05, max_jitter=4, seed=0, device="cuda", init=0.5,
                 eot_scale=(1.0, 1.0), eot_rotation=0.0, eot_contrast=0.0, eot_brightness=0.0):
        if placement not in PLACEMENTS:
            raise ValueError(f"placement {placement!r} not in {PLACEMENTS}")
        self.image_hw, self.patch_hw = tuple(int(v) for v in image_hw), tuple(int(v) for v in patch_hw)
        self.placement, self.x0, self.y0 = placement, int(x0), int(y0)
        self.eps = None if eps is None else float(eps)
        self.eot_translations, self.max_jitter, self.lr = int(eot_translations), int(max_jitter), float(lr)
        self.generator = torch.Generator().manual_seed(int(seed))
        self.eot_ranges = (tuple(float(v) for v in eot_scale), float(eot_rotation), float(eot_contrast),
                           float(eot_brightness))
        self.transformed = _check_ranges(*self.eot_ranges, self.eot_translations)
        self.transform_generator = torch.Generator().manual_seed(int(seed) + TRANSFORM_SEED_OFFSET)
        self._host_offsets = None  # the last offsets() on the host, for transforms()
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
        self._host_offsets = eot_offsets(self.offset, n, copies, self.generator, self.max_jitter)
        return self._host_offsets.to(self.patch.device)

    def transforms(self, n, jitter=True, offsets=None):
        """(n * (1 + eot_translations), 8) f32 device rows (transform_rows) for a batch of n images, or None when
        every range is off (or jitter is False: the identity). The rows are centred on `offsets` (a host tensor);
        None: on what the last offsets() call returned if it has as many rows (kept on the host, so nothing is read
        back from the device), else on the base offset. Draws from transform_generator only."""
        if not (self.transformed and jitter):
            return None
        rows = n * (1 + self.eot_translations)
        if offsets is None:
            last = self._host_offsets
            offsets = last if last is not None and last.shape[0] == rows else \
                torch.tensor(self.offset, dtype=torch.int32).repeat(rows, 1)
        params = eot_transforms(n, self.eot_translations, self.transform_generator, *self.eot_ranges)
        return transform_rows(offsets, params, self.patch_hw).to(self.patch.device)

    def apply(self, images, offsets, need_f32=True, transforms=None):
        """images (..., H, W, C) uint8 or f32 in [0, 1], offsets (N, 2) for the N = prod(...) images -> (composited
        f32 images or None, the encoder input: - 0.5, channel-padded), both with the leading shape of `images`.
        transforms (N, 8) rows: the patch is resampled through them (they carry the offsets; `offsets` is not read)."""
        lead = images.shape[:-3]
        flat = images.reshape(-1, *images.shape[-3:]).contiguous()
        if transforms is None:
            f, enc = K.patch_apply(flat, self.patch, offsets, need_f32=need_f32)
        else:
            f, enc = K.patch_apply_affine(flat, self.patch, transforms, need_f32=need_f32)
        return (None if f is None else f.view(*lead, *f.shape[-3:])), enc.view(*lead, *enc.shape[-3:])

    def grad(self, d_image, offsets, w_tv=0.0, transforms=None):
        """(d_patch, tv): the image gradient folded onto the patch (+ w_tv * d TV / d patch), and the patch's TV;
        transforms as in apply (the adjoint of the resampling compositor)"""
        flat = d_image.reshape(-1, *d_image.shape[-3:]).contiguous()
        if transforms is None:
            return K.patch_grad(flat, offsets, self.patch_hw, patch=self.patch, w_tv=w_tv)
        return K.patch_grad_affine(flat, transforms, self.patch_hw, patch=self.patch, w_tv=w_tv)

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


def attack_gradient(agent, patch, loss, data, initial, seed, offsets, clean=None, transforms=None):
    """One evaluation of the objective on a batch with the patch at `offsets` (N * copies rows: the batch is tiled to
    match, and a PlanningAttackLoss imagines from the tiled rows), resampled through `transforms` when given
    (AdversarialPatch.transforms): -> (loss, terms, d_image, clean). No parameter gradient is written
    (ops.grad_sink_scope)."""
    B, T = data["action"].shape[:2]
    copies = offsets.shape[0] // (B * T) - 1
    tiled = {k: _tile(v, copies) for k, v in data.items() if k != "__enc_image"}
    init = tuple(_tile(t, copies) for t in initial)
    if clean is None:
        clean = loss.clean(agent, agent.posterior(tiled, init, seed=seed))
    img, _ = patch.apply(tiled["image"], offsets, transforms=transforms)
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


def _refuse_unsupported(agent):
    if agent.rep_loss == "dreamerpro":
        raise NotImplementedError("the patch attack with rep_loss=dreamerpro")
    if getattr(agent, "world", 1) > 1:
        raise NotImplementedError("the patch attack under data parallel")


def _patch_from_config(cfg, image_hwc, device, seed, init=0.5):
    H, W, C = image_hwc
    return AdversarialPatch((H, W), C, tuple(cfg.patch_hw), cfg.placement, cfg.get("x0", 0), cfg.get("y0", 0),
                            cfg.eps, cfg.eot_translations, cfg.lr, int(cfg.get("max_jitter", 4)), seed,
                            device=device, init=init, **dict(zip(EOT_RANGE_KEYS, eot_ranges(cfg))))


def train_patch(agent, batches, cfg, patch=None):
    """Optimise a patch against `agent` on `batches` (a list of (data, initial); data a dict of (B, T, *) device
    tensors, image uint8 or f32) for cfg.steps steps -> (patch (ph, pw, C), log (steps, 4)): the objective's terms
    per step in LOG_KEYS order (with cfg.w_return != 0: (steps, 5), LOG_KEYS_PLANNING, and the objective is
    PlanningAttackLoss), a device tensor (no host synchronisation in the loop). Step i uses batch i mod
    len(batches) with the posterior noise of seed cfg.seed + that batch's index; its clean posterior is computed
    once. With an eot_* range on, every EoT copy is also scaled / rotated / re-lit (AdversarialPatch.transforms); with
    all of them off the loop launches exactly what it launches without them."""
    _refuse_unsupported(agent)
    loss = make_loss(cfg)
    planning = isinstance(loss, PlanningAttackLoss)
    img0 = batches[0][0]["image"]
    B, T, H, W, C = img0.shape
    seed = int(cfg.get("seed", 0))
    if patch is None:
        patch = _patch_from_config(cfg, (H, W, C), img0.device, seed)
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
        rows = patch.transforms(B * T)  # None unless an eot_* range is on
        total, terms, d_image, cleans[j] = attack_gradient(agent, patch, loss, data, initial, seed + j, offsets,
                                                           cleans.get(j), transforms=rows)
        d_patch, tv = patch.grad(d_image, offsets, loss.w_tv, transforms=rows)
        log[i, 0], log[i, 1], log[i, 2], log[i, 3] = total + loss.w_tv * tv[0], terms["kl"], terms["action"], tv[0]
        if planning:
            log[i, 4] = terms["ret"]
        patch.step(d_patch)
    return patch.patch, log


# ------------------------------------------------------------------------------------------------- evaluation
def _as_patch(patch, cfg, image_hwc, device, seed):
    """an AdversarialPatch as it is; a (ph, pw, C) tensor placed by cfg (saliency: the centre)"""
    if isinstance(patch, AdversarialPatch):
        return patch
    cfg = Config({**cfg, "patch_hw": list(patch.shape[:2])})
    return _patch_from_config(cfg, image_hwc, device, seed, init=patch)


def evaluation_rows(patch, n, generator, cfg):
    """(n, 8) host rows for evaluate_patch(transforms=True): every image its own offset jitter (cfg.max_jitter) and
    its own draw from cfg's eot_* ranges (no identity copy), both from `generator`, the jitter first"""
    jitter = eot_offsets(patch.offset, n, 1, generator, int(cfg.get("max_jitter", 4)))[n:]
    ranges = eot_ranges(cfg, copies=1)
    return transform_rows(jitter, eot_transforms(n, 1, generator, *ranges)[n:], patch.patch_hw)


@torch.no_grad()
def evaluate_patch(agent, batches, patch, cfg, seed=None, transforms=False):
    """Clean against patched on replay batches -> (len(batches), 4) device tensor, columns EVAL_KEYS: mean(ret0) of
    Dreamer.imagined_return (cfg.horizon) from the clean and from the patched posterior, KL(clean || patched) and the
    actor-mode shift (PosteriorAttackLoss's terms). Batch j is observed and imagined with the noise of seed
    cfg.seed + j, as train_patch does. patch: an AdversarialPatch, or a (ph, pw, C) tensor placed by cfg. The patch
    sits at its base offset on every frame; transforms=True: every frame gets its own jitter and its own draw from
    cfg's eot_* ranges instead (evaluation_rows), from a generator seeded by `seed` (None: cfg.seed) — a seed the
    training did not use evaluates robustness on held-out transformations. No gradient, no parameter gradient, no host
    synchronisation."""
    _refuse_unsupported(agent)
    img0 = batches[0][0]["image"]
    B, T, H, W, C = img0.shape
    base_seed = int(cfg.get("seed", 0))
    patch = _as_patch(patch, cfg, (H, W, C), img0.device, base_seed)
    loss = PosteriorAttackLoss(1.0, 1.0, 0.0)
    horizon = cfg.get("horizon", None)
    generator = torch.Generator().manual_seed(base_seed if seed is None else int(seed))
    out = torch.zeros(len(batches), len(EVAL_KEYS), dtype=torch.float32, device=img0.device)
    for j, (data, initial) in enumerate(batches):
        data = {k: v for k, v in data.items() if k != "__enc_image"}
        sj = base_seed + j
        rows = evaluation_rows(patch, B * T, generator, cfg).to(img0.device) if transforms else None
        post = agent.posterior(data, initial, seed=sj)
        clean = loss.clean(agent, post)
        img, _ = patch.apply(data["image"], patch.offsets(B * T, jitter=False), transforms=rows)
        adv = agent.posterior({**data, "image": img}, initial, seed=sj)
        _, terms = loss(agent, clean, *adv)
        out[j, 0] = agent.imagined_return(post[0], post[1], horizon, seed=sj).mean()
        out[j, 1] = agent.imagined_return(adv[0], adv[1], horizon, seed=sj).mean()
        out[j, 2], out[j, 3] = terms["kl"], terms["action"]
    return out


@torch.no_grad()
def patched_act(agent, patch, obs, state, eval=False, seed=None, step=0, offsets=None, transforms=None):
    """Dreamer.act on observations that carry the patch: obs["image"] (B, H, W, C) uint8 or f32 is composited
    (offsets (B, 2) int32 device rows, None: the patch's base offset; transforms (B, 8): resampled through them) and
    the agent acts on the result -> (action, state) as Dreamer.act."""
    image = obs["image"]
    if offsets is None:
        offsets = patch.offsets(image.shape[0], jitter=False)
    img, _ = patch.apply(image, offsets, transforms=transforms)
    return agent.act({**obs, "image": img}, state, eval=eval, seed=seed, step=step)


def patched_policy_graph(agent, patch, B, obs_example, eval=False, transforms=None):
    """patched_act for B environments as one replayed HIP graph, in the manner of Dreamer.policy_graph: returns
    policy(obs, state) -> (action, state), views of the graph's static outputs. Call k equals
    patched_act(..., seed=seed_base + k, step=0). The patch (patch.patch), the offsets (policy.offsets, the base
    offset) and the rows (policy.transforms, a copy of `transforms`, or None) are static device buffers the graph
    reads in place: a patch stepped between calls, or offsets / rows copied into those buffers, are seen without a
    new capture."""
    dev = agent.device
    s_obs = {k: torch.zeros_like(v, device=dev) for k, v in obs_example.items()}
    s_state = agent.get_initial_state(B)
    seed_dev = torch.zeros(1, dtype=torch.int64, device=dev)
    s_offsets = patch.offsets(B, jitter=False)
    s_rows = None if transforms is None else transforms.to(dev).clone()
    if agent._mm:  # as Dreamer.policy_graph: the act-side context buffer exists before the capture
        agent.encoder.act_context(B, dev, eval=eval)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        act, st = patched_act(agent, patch, s_obs, s_state, eval=eval, seed=seed_dev, step=0, offsets=s_offsets,
                              transforms=s_rows)
    counter = [0]
    base = agent._seed_base + 7

    def policy(obs, state):
        for k, v in obs.items():
            s_obs[k].copy_(v)
        for k in ("stoch", "deter", "prev_action"):
            s_state[k].copy_(state[k])
        seed_dev.fill_(base + counter[0])
        counter[0] += 1
        if agent._mm:
            agent.encoder.act_context(B, dev, eval=eval)
        g.replay()
        return act, st

    policy.graph, policy.counter, policy.offsets, policy.transforms = g, counter, s_offsets, s_rows
    return policy
