"""sdreamer.attack.train_patch on the walker_r2 weights, judged by the CPU oracle (tests/attack_ref.py)."""
import numpy as np
import pytest
import torch

import attack_ref as ar
from golden_io import batch, initial, load_case
from test_gpu_dreamer import build_agent

pytestmark = pytest.mark.gpu
DEV = "cuda"
STEPS, LR = 20, 0.05


def _cfg(**kw):
    from sdreamer.attack import load_attack_config
    base = dict(w_kl=ar.W_KL, w_action=ar.W_ACTION, w_tv=ar.W_TV, steps=STEPS, lr=LR, seed=ar.SEED,
                placement=ar.PLACEMENT, eot_translations=0)
    base.update(kw)
    return load_attack_config([f"{k}={v}" for k, v in base.items()])


def test_train_patch_raises_the_oracle_objective():
    """train_patch at B2 T6 with w_kl = 1, w_action = 1, w_tv = 0.01 from a gray patch at bottom_center; the objective
    w_kl * KL(clean || patched) + w_action * (actor-mode shift), evaluated by the oracle on the CPU, must be larger
    for the returned patch than for the initial one.

    Step count and lr come from the same loop on the oracle alone (tests/attack_ref.py: oracle autograd,
    torch.optim.Adam, the same seeds). Its objective relative to the initial patch's 0.12921 (KL 0.11569, shift
    0.013515) after steps 1..20:
      eot 2  lr 0.02: 0.96 1.01 0.98 0.97 0.97 0.99 1.06 1.07 1.08 1.08 1.10 1.09 1.12 1.11 1.13 1.09 1.14 1.16 1.16 1.15
      eot 2  lr 0.05: 0.80 0.85 0.87 0.94 0.95 0.98 1.04 1.11 1.08 1.08 1.12 1.09 1.16 1.23 1.22 1.24 1.24 1.24 1.24 1.23
      eot 2  lr 0.1 : 0.68 0.73 0.77 0.87 0.90 0.96 0.93 0.95 1.04 1.16 1.12 1.14 1.14 1.13 1.13 1.15 1.21 1.22 1.25 1.27
      eot 0  lr 0.02: 0.93 1.08 1.06 1.06 1.09 1.11 1.14 1.17 1.17 1.19 1.20 1.25 1.28 1.28 1.27 1.27 1.27 1.27 1.28 1.30
      eot 0  lr 0.05: 0.75 0.85 0.91 0.96 0.99 1.07 1.09 1.14 1.11 1.16 1.23 1.27 1.27 1.30 1.30 1.31 1.32 1.31 1.29 1.31
      eot 0  lr 0.1 : 0.62 0.71 0.72 0.81 0.93 0.92 0.96 1.02 1.06 1.11 1.14 1.20 1.22 1.32 1.37 1.34 1.31 1.33 1.37 1.36
    With eot_translations = 2 the oracle clears the condition at no lr by the factor of 2 that was asked of it, so
    eot_translations is 0 here (the EoT path has its own test below). Without EoT it does not reach 2 either within 20
    steps (best 1.37): a gray patch on these random-noise frames already shifts the posterior (the objective of an
    all-ones patch, 0.209, is 1.6 of it), and the straight-through gradient of the sampled latents makes the first Adam
    steps lose ground. The run used is eot 0, lr 0.05, 20 steps: above 1.2 from step 11 on, 1.31 at the end. The
    assertion is the condition itself; the measured ratio of the GPU run is printed (MI355X: 0.12921 -> 0.17459,
    1.35; the product's first logged step equals the oracle's initial terms to five digits)."""
    from sdreamer.attack import train_patch
    ag, z, spec, obs = build_agent("walker_r2")
    data, init = batch(z, 0, obs, DEV), initial(z, 0, spec, DEV)
    patch, log = train_patch(ag, [(data, init)], _cfg())
    torch.cuda.synchronize()
    assert patch.shape == (16, 16, 3) and log.shape == (STEPS, 4)
    assert bool(torch.isfinite(log).all()) and float(patch.min()) >= 0.0 and float(patch.max()) <= 1.0
    assert all(p.grad is None or not bool(p.grad.any()) for p in ag.parameters())
    params = load_case("walker_r2")[3]
    cpu = batch(z, 0, obs), initial(z, 0, spec)
    offset = (48, 24)
    first = ar.objective(spec, params, *cpu, ar.SEED, torch.full((16, 16, 3), 0.5), offset)
    last = ar.objective(spec, params, *cpu, ar.SEED, patch.cpu(), offset)
    print(f"oracle objective: initial {first[0]:.5f} (kl {first[1]:.5f}, action {first[2]:.6f}) -> returned "
          f"{last[0]:.5f} (kl {last[1]:.5f}, action {last[2]:.6f}), ratio {last[0] / first[0]:.3f}", flush=True)
    # the first logged step is the initial patch's objective on the product, the oracle's up to the posterior's
    # accuracy: logits within 1e-4 (test_update_matches_reference's bound) move the KL by at most 1e-4 * sum |p - q|
    # <= 1e-4 * 2 * 32 latents; the actor-mode shift within 5 %
    kl0, act0 = float(log[0, 1]), float(log[0, 2])
    print(f"product's first step: kl {kl0:.5f}, action {act0:.6f}", flush=True)
    assert abs(kl0 - first[1]) <= 6.4e-3 and abs(act0 - first[2]) <= 0.05 * first[2], (kl0, act0, first)
    assert last[0] > first[0]


def test_train_patch_eot_saliency_and_eps_paths():
    """Two steps with eot_translations = 2 (the batch tiled three times, jittered offsets), saliency placement and an
    eps ball: finite terms, the patch inside the ball around its start, and the same bits on repetition."""
    from sdreamer.attack import train_patch
    ag, z, spec, obs = build_agent("walker_r2")
    data, init = batch(z, 0, obs, DEV), initial(z, 0, spec, DEV)
    data["image"] = torch.from_numpy(z["u0_in_image"]).to(DEV)  # uint8 frames
    outs = []
    for _ in range(2):
        patch, log = train_patch(ag, [(data, init)], _cfg(steps=2, eot_translations=2, placement="saliency",
                                                          eps=0.03))
        outs.append((patch.clone(), log.clone()))
    torch.cuda.synchronize()
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    patch, log = outs[0]
    assert bool(torch.isfinite(log).all()) and float(log[:, 1].min()) > 0
    d = (patch - 0.5).abs()
    assert float(d.max()) <= 0.03 + 1e-7 and float(d.max()) > 0
    assert np.isfinite(float(log.sum()))
