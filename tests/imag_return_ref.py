"""The imagined-return objective on the CPU oracle (oracle/ref_cpu.py) under autograd: the reference of
Dreamer.imagined_return and its backward (ops.ImagineReturnFn). Test infrastructure, not a test.

Oracle.imagine is no_grad, so the rollout is restated here as a loop over the oracle's own functions (get_feat,
head_logits, actor_sample, deter_step, img_logit, sample_stoch, twohot_mode): the same noise streams, counters and
hard samples, gradients as upstream's modules pass them (straight-through Gumbel-softmax samples, the bounded normal's
reparameterisation, the action's normalisation a division by a constant, every parameter frozen). The lambda-return
is a differentiable copy of ref_cpu.lambda_return's recurrence (that function is no_grad). ref_cpu.DT is read at call
time (small_models.oracle_dtype), so everything runs in float32 or float64.

    python tests/imag_return_ref.py      the planning attack's loop on the oracle alone (walker_r2 golden weights)
"""
import os
import sys

import numpy as np
import torch

if __name__ == "__main__":
    _root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path[:0] = [_root, os.path.join(_root, "tests"), os.path.join(_root, "safe-dreamer_amd")]

from oracle import noise as nz  # noqa: E402
from oracle import ref_cpu  # noqa: E402

MUTATIONS = ("no_straight_through", "no_cont_grad", "eps_zero")


def lambda_return_diff(term, reward, value, boot, disc, lamb):
    """ref_cpu.lambda_return with last = 0, under autograd (the same expressions in the same order)"""
    live = (1 - term)[:, 1:] * disc
    cont = torch.ones_like(live) * lamb
    interm = reward[:, 1:] + (1 - cont) * live * boot[:, 1:]
    out = [boot[:, -1]]
    for i in reversed(range(live.shape[1])):
        out.append(interm[:, i] + live[:, i] * cont[:, i] * out[-1])
    return torch.stack(list(reversed(out))[:-1], 1)


def rollout(orc, start, H1, seed, row_offset=0, mutate=None):
    """Oracle.imagine with the autograd graph kept: feats (N, H1, F), actions (N, H1, A), prior / actor logits."""
    assert mutate in (None,) + MUTATIONS
    s = orc.s
    P = {k: v.detach() for k, v in orc.P.items()}
    stoch, deter = start
    N = deter.shape[0]
    feats, actions, plogits, alogits = [], [], [], []
    for t in range(H1):
        feat = orc.get_feat(stoch, deter)
        alogit = orc.head_logits("actor", feat, P)
        action = orc.actor_sample(alogit, seed, t, row_offset)
        if mutate == "no_straight_through" and s.discrete:
            action = action.detach()
        if mutate == "eps_zero" and not s.discrete:  # the gradient of loc alone: the eps * scale part a constant
            loc, _ = ref_cpu.bounded_normal_params(alogit, float(s.actor_dist.min_std), float(s.actor_dist.max_std))
            action = loc + (action - loc).detach()
        feats.append(feat)
        actions.append(action)
        alogits.append(alogit)
        if t == H1 - 1:
            break
        deter = orc.deter_step(stoch, deter, action, P)
        g = torch.from_numpy(nz.gumbel_block(seed, nz.STREAM_IMG, t, N, row_offset, s.SK))
        ilogit = orc.img_logit(deter, P)
        stoch = orc.sample_stoch(ilogit, g.reshape(N, s.S, s.K))
        if mutate == "no_straight_through":
            stoch = stoch.detach()
        plogits.append(ilogit)
    return torch.stack(feats, 1), torch.stack(actions, 1), plogits, alogits


def returns(orc, feats, mutate=None):
    """the heads on every feat and the lambda-return: dict(reward, cont, value, ret), (N, H1) and ret (N, H1 - 1)"""
    c = orc.s.cfg
    P = {k: v.detach() for k, v in orc.P.items()}
    reward = ref_cpu.twohot_mode(orc.head_logits("reward", feats, P), orc.rbins).squeeze(-1)
    cont = torch.sigmoid(orc.head_logits("cont", feats, P).to(ref_cpu.DT)).squeeze(-1)
    value = ref_cpu.twohot_mode(orc.head_logits("value", feats, P), orc.bins).squeeze(-1)
    if mutate == "no_cont_grad":
        cont = cont.detach()
    disc = 1 - 1 / int(c.horizon)
    ret = lambda_return_diff(1 - cont, reward, value, value, disc, float(c.lamb))
    return dict(reward=reward, cont=cont, value=value, ret=ret, disc=disc, lamb=float(c.lamb))


def imagined_return(orc, stoch0, deter0, H1, seed, row_offset=0, u=None, mutate=None):
    """ret0 (N,) of the rollout from (stoch0 (N, S, K), deter0 (N, D)) and the gradient of sum(ret0 * u) (u None:
    ones) to the start state. -> dict of numpy float64 arrays: ret0, ret, reward, cont, value, feats (H1, N, F) and
    actions (H1, N, A) time-major, idx (H1, N, S), d_stoch (N, S, K), d_deter (N, D), and the logits the margins
    need (prior_logit (N, H1 - 1, S, K), actor_logit (N, H1, A'))."""
    DT = ref_cpu.DT
    s0 = stoch0.to(DT).clone().requires_grad_(True)
    d0 = deter0.to(DT).clone().requires_grad_(True)
    feats, actions, plogits, alogits = rollout(orc, (s0, d0), H1, seed, row_offset, mutate)
    rr = returns(orc, feats, mutate)
    ret0 = rr["ret"][:, 0]
    w = torch.ones_like(ret0) if u is None else torch.as_tensor(u, dtype=DT)
    gs, gd = torch.autograd.grad((ret0 * w).sum(), [s0, d0])
    f64 = lambda t: t.detach().numpy().astype(np.float64)  # noqa: E731
    SK = orc.s.SK
    ft = feats.detach().transpose(0, 1)
    out = dict(ret0=f64(ret0), ret=f64(rr["ret"]), reward=f64(rr["reward"]), cont=f64(rr["cont"]),
               value=f64(rr["value"]), feats=f64(ft), actions=f64(actions.transpose(0, 1)),
               idx=ft[..., :SK].reshape(H1, ft.shape[1], orc.s.S, orc.s.K).argmax(-1).numpy(),
               d_stoch=f64(gs), d_deter=f64(gd), actor_logit=f64(torch.stack(alogits, 1)))
    if plogits:
        out["prior_logit"] = f64(torch.stack(plogits, 1))
    return out


# --------------------------------------------------------------------------------------------- the planning attack
# W_TV = 0 in the return-lowering test: on these random-weight frames mean(ret0) is about 3e-3 and its patch gradient
# is orders of magnitude below the TV term's 0.01 per neighbour difference, which then steers Adam alone (main()
# prints both loops: with w_tv = 0.01 the oracle's own return wanders and ends above the gray patch's)
PATCH_HW, PLACEMENT, SEED, MAX_JITTER, W_TV = (16, 16), "bottom_center", 0, 4, 0.0


class OraclePlanning:
    """mean(ret0) of a patch on one batch (tiled for the EoT copies): encoder -> posterior -> imagined return"""

    def __init__(self, spec, params, data, init, seed, copies=0, horizon=None):
        from attack_ref import _tile
        self.M = ref_cpu.OracleAgent(spec, params).model
        self.spec, self.seed = spec, seed
        self.data = {k: _tile(v, copies) for k, v in data.items()}
        self.init = tuple(_tile(t, copies) for t in init)
        self.H1 = (int(spec.cfg.imag_horizon) if horizon is None else int(horizon)) + 1

    def posterior(self, image):
        M, d = self.M, self.data
        return M.observe(M.encode({**d, "image": image.to(ref_cpu.DT)}), d["action"].to(ref_cpu.DT),
                         tuple(t.to(ref_cpu.DT) for t in self.init), d["is_first"], self.seed)

    def ret0_of_image(self, image):
        s = self.spec
        ps, pd, _ = self.posterior(image)
        feats, _, plogits, alogits = rollout(self.M, (ps.reshape(-1, s.S, s.K), pd.reshape(-1, s.D)), self.H1,
                                             self.seed)
        self.last_logits = (plogits, alogits)
        return returns(self.M, feats)["ret"][:, 0]

    def mean_ret(self, patch, offsets):
        from attack_ref import composite
        img = self.data["image"]
        flat = composite(img.reshape(-1, *img.shape[-3:]), patch, offsets)
        return self.ret0_of_image(flat.view(img.shape)).mean()


def objective(spec, params, data, init, seed, patch, offset, dtype=torch.float64):
    """mean(ret0) of `patch` at the base offset on every frame (no jitter), no grad, in `dtype`, as a float"""
    B, T = data["action"].shape[:2]
    old, ref_cpu.DT = ref_cpu.DT, dtype
    try:
        cast = lambda v: v.to(dtype) if v.is_floating_point() else v  # noqa: E731
        att = OraclePlanning(spec, params, {k: cast(v) for k, v in data.items()}, tuple(cast(t) for t in init), seed)
        with torch.no_grad():
            return float(att.mean_ret(patch.to(dtype), torch.tensor([offset] * (B * T))))
    finally:
        ref_cpu.DT = old


def oracle_train(spec, params, data, init, steps, lr, eot, w_tv=W_TV):
    """the planning attack's loop (w_return 1, w_kl 0, w_action 0) on the oracle alone: autograd, torch.optim.Adam,
    the seeds and jitter draws of sdreamer.attack.train_patch -> the patch after every step"""
    from attack_ref import tv
    from sdreamer.attack import eot_offsets, placement_offset
    B, T, H, W, C = data["image"].shape
    offset = placement_offset(PLACEMENT, (H, W), PATCH_HW)
    gen = torch.Generator().manual_seed(SEED)
    att = OraclePlanning(spec, params, data, init, SEED, eot)
    patch = torch.full((*PATCH_HW, C), 0.5).requires_grad_()
    opt = torch.optim.Adam([patch], lr=lr)
    out = []
    for _ in range(steps):
        offs = eot_offsets(offset, B * T, eot, gen, MAX_JITTER)
        loss = att.mean_ret(patch, offs) + w_tv * tv(patch)
        opt.zero_grad()
        loss.backward()
        opt.step()
        with torch.no_grad():
            patch.clamp_(0.0, 1.0)
        out.append(patch.detach().clone())
    return offset, out


def main():
    from golden_io import batch, initial, load_case
    torch.set_num_threads(8)
    z, cfg, spec, params, obs = load_case("walker_r2")
    data, init = batch(z, 0, obs), initial(z, 0, spec)
    for w_tv in (W_TV, 0.01):
        for eot in (0, 2):
            offset, patches = oracle_train(spec, params, data, init, 20, 0.05, eot, w_tv)
            first = objective(spec, params, data, init, SEED, torch.full((*PATCH_HW, 3), 0.5), offset)
            vals = [objective(spec, params, data, init, SEED, p, offset) for p in patches]
            print(f"w_tv {w_tv} eot {eot} lr 0.05: mean(ret0) gray patch {first:.6f}; after steps 1..20: "
                  + " ".join(f"{v:.6f}" for v in vals), flush=True)


if __name__ == "__main__":
    main()
