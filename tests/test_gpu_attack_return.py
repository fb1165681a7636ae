"""The planning-level attack end to end on the walker_r2 weights (B2 T6): d mean(ret0) / d image through the encoder,
the posterior and the imagination against the float64 oracle, train_patch with w_return judged by the oracle
(tests/imag_return_ref.py), and the w_return = 0 path left bit for bit as it was."""
import numpy as np
import pytest
import torch

import imag_return_ref as irr
import imgrad_ref as ir
import small_models as sm
from golden_io import batch, initial, load_case
from test_gpu_dreamer import build_agent
from test_gpu_imgrad import _check

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS, LR = 20, 0.05
# the first k of 0, 1, 2, ... at which the float32 oracle's posterior samples (STREAM_OBS) and imagined prior samples
# (STREAM_IMG) of this batch all have a top-2 margin >= 2e-4 with noise seed k; found on the CPU from the oracle alone
# (the actor is a bounded normal: no action index)
K_SEED = 0
# mean(ret0) in float64 of the oracle's own loop with w_tv = 0 (python tests/imag_return_ref.py): gray patch, after
# 20 steps, by EoT copies
ORACLE_RUN = {0: (-0.002825, -0.003440), 2: (-0.002825, -0.003676)}


def _cfg(**kw):
    from sdreamer.attack import load_attack_config
    base = dict(w_return=1.0, w_kl=0.0, w_action=0.0, w_tv=irr.W_TV, steps=STEPS, lr=LR, seed=irr.SEED,
                placement=irr.PLACEMENT, eot_translations=0)
    base.update(kw)
    return load_attack_config([f"{k}={v}" for k, v in base.items()])


def test_image_gradient_of_the_imagined_return_matches_float64():
    """d mean(ret0) / d image of Dreamer.observation_grad with Dreamer.imagined_return as the loss, against the
    oracle in float64 under autograd (encoder -> observe -> the rollout of imag_return_ref), on test_gpu_imgrad.py's
    bounds: per-frame norms within 2e-4, 4,096 sampled elements within 2e-3 relative + 1e-4 of the largest."""
    from parity import imag_margins, post_margins
    ag, z, spec, obs = build_agent("walker_r2")
    data, init = batch(z, 0, obs, DEV), initial(z, 0, spec, DEV)
    keep = {}

    def loss_fn(ps, pd, pl):
        keep["post_idx"] = ps.detach().argmax(-1).cpu().numpy()
        return ag.imagined_return(ps, pd, seed=K_SEED, keep=keep).mean()

    loss, g = ag.observation_grad(data, init, loss_fn, seed=K_SEED)
    torch.cuda.synchronize()
    assert all(p.grad is None or not bool(p.grad.any()) for p in ag.parameters())
    params = load_case("walker_r2")[3]
    cpu, cini = batch(z, 0, obs), initial(z, 0, spec)
    with sm.oracle_dtype(torch.float32):  # the input condition, on the float32 oracle
        a32 = irr.OraclePlanning(spec, params, cpu, cini, K_SEED)
        with torch.no_grad():
            _, _, pl32 = a32.posterior(cpu["image"])
            a32.ret0_of_image(cpu["image"])
        assert float(post_margins(pl32.numpy(), K_SEED, spec.unimix).min()) >= 2e-4
        assert float(imag_margins(torch.stack(a32.last_logits[0], 1).numpy(), K_SEED, spec.unimix, 0).min()) >= 2e-4
    with sm.oracle_dtype(torch.float64):
        att = irr.OraclePlanning(spec, params, cpu, cini, K_SEED)
        img = cpu["image"].double().requires_grad_()
        ps, pd, _ = att.posterior(img)
        feats, _, _, _ = irr.rollout(att.M, (ps.reshape(-1, spec.S, spec.K), pd.reshape(-1, spec.D)), att.H1, K_SEED)
        ref = irr.returns(att.M, feats)["ret"][:, 0].mean()
        ref.backward()
    assert np.array_equal(keep["post_idx"], ps.detach().argmax(-1).numpy())
    SK = spec.S * spec.K
    idx = keep["feats"][..., :SK].reshape(att.H1, -1, spec.S, spec.K).argmax(-1).cpu().numpy()
    assert np.array_equal(idx, feats.detach().transpose(0, 1)[..., :SK].reshape(idx.shape + (spec.K,)).argmax(-1).numpy())
    ref = float(ref.detach())
    print(f"mean(ret0): product {float(loss):.6f}, float64 oracle {ref:.6f}", flush=True)
    assert abs(float(loss) - ref) <= sm.IMAG_ATOL + sm.IMAG_RTOL * abs(ref)
    assert float(np.abs(img.grad.numpy()).max()) > 0
    _check(g, *ir.sampled(img.grad.numpy()), "walker_r2 d mean(ret0) / d image")


@pytest.mark.parametrize("eot", [0, 2])
def test_train_patch_lowers_the_oracle_imagined_return(eot):
    """train_patch with w_return = 1, w_kl = 0, w_action = 0, 20 steps at lr 0.05 from a gray patch at bottom_center,
    without and with 2 EoT copies. mean(ret0) of the returned patch, evaluated by the oracle in float64 without grad
    (no jitter), must be lower than the gray patch's by half of what the same loop on the oracle alone achieves.

    The oracle's own loop (python tests/imag_return_ref.py: oracle autograd, torch.optim.Adam, the same seeds and
    jitter draws), mean(ret0) from the gray patch's -0.002825 after steps 1..20:
      w_tv 0    eot 0: -0.003213 -0.002682 -0.003071 -0.003116 -0.003024 -0.002795 -0.003272 -0.003338 -0.003408 -0.003544
                       -0.003387 -0.003494 -0.003494 -0.003813 -0.003813 -0.003813 -0.003440 -0.003440 -0.003440 -0.003440
      w_tv 0    eot 2: -0.002956 -0.002622 -0.003155 -0.003527 -0.003240 -0.003206 -0.003508 -0.003584 -0.003584 -0.003908
                       -0.003845 -0.003541 -0.003661 -0.003657 -0.003657 -0.003657 -0.003657 -0.003657 -0.003657 -0.003676
      w_tv 0.01 eot 0: -0.003213 -0.002818 -0.002892 -0.002689 -0.002742 -0.002653 -0.002811 -0.002829 -0.002245 -0.002561
                       -0.002637 -0.002501 -0.002262 -0.002789 -0.002667 -0.002940 -0.002761 -0.002576 -0.002468 -0.002640
      w_tv 0.01 eot 2: -0.002956 -0.002945 -0.003117 -0.002863 -0.002982 -0.002906 -0.002821 -0.002645 -0.002488 -0.002871
                       -0.002719 -0.002818 -0.002933 -0.002625 -0.002625 -0.002625 -0.002719 -0.002911 -0.002476 -0.002303
    With the configuration's default w_tv = 0.01 the oracle's own loop does not lower the return: on these
    random-weight frames the return is about 3e-3 and its patch gradient far below the TV term's 0.01 per neighbour
    difference, so after the first step Adam follows the TV term (the product's loop with w_tv = 0.01 ends at the
    oracle's -0.002640 / -0.002303 to six digits: faithful, and not lower either). The weight of the TV term is this
    test's to choose, and it is about the return term, so w_tv = 0 here: the oracle's loop then drops the return by
    0.000615 (eot 0) and 0.000851 (eot 2), and half of that is required of the product. The TV path of the loop is
    covered by tests/test_gpu_attack.py and the bit-for-bit test below."""
    from sdreamer.attack import LOG_KEYS_PLANNING, train_patch
    ag, z, spec, obs = build_agent("walker_r2")
    data, init = batch(z, 0, obs, DEV), initial(z, 0, spec, DEV)
    patch, log = train_patch(ag, [(data, init)], _cfg(eot_translations=eot))
    torch.cuda.synchronize()
    assert patch.shape == (16, 16, 3) and log.shape == (STEPS, 5) and len(LOG_KEYS_PLANNING) == 5
    assert bool(torch.isfinite(log).all()) and float(patch.min()) >= 0.0 and float(patch.max()) <= 1.0
    assert not bool(log[:, 1].any()) and not bool(log[:, 2].any())  # the KL and action terms are off
    assert all(p.grad is None or not bool(p.grad.any()) for p in ag.parameters())
    params = load_case("walker_r2")[3]
    cpu = batch(z, 0, obs), initial(z, 0, spec)
    offset = (48, 24)
    first = irr.objective(spec, params, *cpu, irr.SEED, torch.full((16, 16, 3), 0.5), offset)
    last = irr.objective(spec, params, *cpu, irr.SEED, patch.cpu(), offset)
    o_first, o_last = ORACLE_RUN[eot]
    print(f"eot {eot}: oracle mean(ret0) gray {first:.6f} -> returned patch {last:.6f} (drop {first - last:.6f}; the "
          f"oracle's own loop: {o_first:.6f} -> {o_last:.6f}); product's first logged ret {float(log[0, 4]):.6f}",
          flush=True)
    assert abs(first - o_first) <= 5e-6
    if eot == 0:  # the first logged step is the gray patch's return on the product (no jitter without EoT)
        assert abs(float(log[0, 4]) - first) <= sm.IMAG_ATOL + sm.IMAG_RTOL * abs(first)
    assert o_first - o_last > 0
    assert first - last >= 0.5 * (o_first - o_last)


def test_all_terms_with_eot_and_saliency_placement():
    """Two steps with every term on (w_return, w_kl, w_action, w_tv), eot_translations = 2 (the imagination runs from
    the tiled rows), saliency placement (the seeded perturbation, taken with the planning loss) and uint8 frames:
    finite terms in 5 columns, a positive KL, and the same bits on repetition."""
    from sdreamer.attack import train_patch
    ag, z, spec, obs = build_agent("walker_r2")
    data, init = batch(z, 0, obs, DEV), initial(z, 0, spec, DEV)
    data["image"] = torch.from_numpy(z["u0_in_image"]).to(DEV)
    outs = []
    for _ in range(2):
        patch, log = train_patch(ag, [(data, init)], _cfg(steps=2, eot_translations=2, placement="saliency", w_kl=1.0,
                                                          w_action=1.0, w_tv=0.01, eps=0.03))
        outs.append((patch.clone(), log.clone()))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    patch, log = outs[0]
    assert log.shape == (2, 5) and bool(torch.isfinite(log).all())
    assert float(log[:, 1].min()) > 0 and bool(log[:, 4].abs().min() > 0)
    # loss = w_return * ret - (w_kl * kl + w_action * action) + w_tv * tv, from the logged terms
    want = log[:, 4] - (log[:, 1] + log[:, 2]) + 0.01 * log[:, 3]
    assert float((log[:, 0] - want).abs().max()) <= 1e-5 * float(want.abs().max())
    d = (patch - 0.5).abs()
    assert 0 < float(d.max()) <= 0.03 + 1e-7
    assert all(p.grad is None or not bool(p.grad.any()) for p in ag.parameters())


def test_without_w_return_the_attack_is_the_posterior_attack_bit_for_bit():
    """w_return = 0: train_patch's patch and log equal those of the posterior-level loop written out here on
    PosteriorAttackLoss (the loop train_patch ran before the planning term existed), and the log keeps 4 columns."""
    from sdreamer import ops
    from sdreamer.attack import AdversarialPatch, PosteriorAttackLoss, train_patch
    ag, z, spec, obs = build_agent("walker_r2")
    data, init = batch(z, 0, obs, DEV), initial(z, 0, spec, DEV)
    cfg = _cfg(w_return=0.0, w_kl=1.0, w_action=1.0, steps=3)
    patch, log = train_patch(ag, [(data, init)], cfg)
    B, T, H, W, C = data["image"].shape
    loss = PosteriorAttackLoss(cfg.w_kl, cfg.w_action, cfg.w_tv)
    pt = AdversarialPatch((H, W), C, tuple(cfg.patch_hw), cfg.placement, 0, 0, cfg.eps, 0, cfg.lr, 4, irr.SEED,
                          device=DEV)
    want = torch.zeros(3, 4, device=DEV)
    clean = loss.clean(ag, ag.posterior(data, init, seed=irr.SEED))
    for i in range(3):
        offsets = pt.offsets(B * T)
        img, _ = pt.apply(data["image"], offsets)
        img.requires_grad_(True)
        with ops.grad_sink_scope():
            post = ag.posterior({**data, "image": img}, init, seed=irr.SEED, with_grad=True)
            total, terms = loss(ag, clean, *post)
            (d_image,) = torch.autograd.grad(total, img)
        d_patch, tv = pt.grad(d_image, offsets, loss.w_tv)
        want[i, 0], want[i, 1], want[i, 2], want[i, 3] = total.detach() + loss.w_tv * tv[0], terms["kl"], \
            terms["action"], tv[0]
        pt.step(d_patch)
    torch.cuda.synchronize()
    assert log.shape == (3, 4)
    assert torch.equal(patch, pt.patch) and torch.equal(log, want)
