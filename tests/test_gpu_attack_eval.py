"""The affine / photometric EoT in train_patch, and a patch evaluated: attack.evaluate_patch against the CPU oracles
(tests/imag_return_ref.py, tests/attack_ref.py) and against its own parts, attack.patched_act against Dreamer.act on a
host-composited observation, attack.patched_policy_graph against patched_act. walker_r2 weights, B2 T6."""
import pytest
import torch

import attack_ref as ar
import imag_return_ref as irr
import small_models as sm
from golden_io import batch, initial, load_case
from launch_trace import recorded as _recorded
from test_gpu_act import _inputs
from test_gpu_dreamer import build_agent

pytestmark = pytest.mark.gpu
DEV = "cuda"
RANGES = dict(eot_scale="[0.8,1.25]", eot_rotation=20.0, eot_contrast=0.2, eot_brightness=0.1)


def _cfg(**kw):
    from sdreamer.attack import load_attack_config
    base = dict(w_kl=1.0, w_action=1.0, w_tv=0.01, steps=2, lr=0.05, seed=ar.SEED, placement=ar.PLACEMENT,
                eot_translations=0)
    base.update(kw)
    return load_attack_config([f"{k}={v}" for k, v in base.items()])


def _snapshot(ag):
    return [(p.detach().clone(), None if p.grad is None else p.grad.detach().clone()) for p in ag.parameters()]


def _untouched(ag, snap):
    for p, (w, g) in zip(ag.parameters(), snap):
        if not torch.equal(p.detach(), w) or (p.grad is None) != (g is None) or \
                (g is not None and not torch.equal(p.grad, g)):
            return False
    return True


def test_train_patch_with_all_four_ranges():
    """Two steps with eot_translations = 2 and scale, rotation, contrast and brightness on, uint8 frames: the resampling
    kernels run (and the plain pair does not), finite log, a positive KL, the same bits on repetition, no parameter
    gradient."""
    from sdreamer.attack import train_patch
    ag, z, spec, obs = build_agent("walker_r2")
    data, init = batch(z, 0, obs, DEV), initial(z, 0, spec, DEV)
    data["image"] = torch.from_numpy(z["u0_in_image"]).to(DEV)
    cfg = _cfg(eot_translations=2, **RANGES)
    outs = []
    for _ in range(2):
        (patch, log), names = _recorded(lambda: train_patch(ag, [(data, init)], cfg))
        outs.append((patch.clone(), log.clone()))
        assert names.count("sd_patch_apply_affine") == 2 and names.count("sd_patch_grad_affine") == 2
        assert "sd_patch_apply" not in names and "sd_patch_grad" not in names
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    patch, log = outs[0]
    assert log.shape == (2, 4) and bool(torch.isfinite(log).all()) and float(log[:, 1].min()) > 0
    assert float(patch.min()) >= 0 and float(patch.max()) <= 1 and float((patch - 0.5).abs().max()) > 0
    assert all(p.grad is None or not bool(p.grad.any()) for p in ag.parameters())


def test_train_patch_by_default_launches_no_resampling_kernel():
    from sdreamer.attack import train_patch
    ag, z, spec, obs = build_agent("walker_r2")
    data, init = batch(z, 0, obs, DEV), initial(z, 0, spec, DEV)
    for kw in (dict(), dict(eot_translations=2)):
        _, names = _recorded(lambda: train_patch(ag, [(data, init)], _cfg(steps=1, **kw)))
        assert "sd_patch_apply" in names and "sd_patch_grad" in names
        assert not [n for n in names if "_affine" in n]


def test_evaluate_patch_matches_the_oracles():
    """A gray patch at bottom_center, transforms=False: ret_clean and ret_patched against the float64 oracle's
    mean(ret0) within IMAG_ATOL + IMAG_RTOL |ref|, kl and action against attack_ref.objective on test_gpu_attack.py's
    bounds (6.4e-3 absolute, 5 % relative); the same bits on a second call; the agent untouched."""
    from sdreamer.attack import EVAL_KEYS, evaluate_patch
    ag, z, spec, obs = build_agent("walker_r2")
    data, init = batch(z, 0, obs, DEV), initial(z, 0, spec, DEV)
    gray = torch.full((16, 16, 3), 0.5, device=DEV)
    cfg = _cfg()
    snap = _snapshot(ag)
    out = evaluate_patch(ag, [(data, init)], gray, cfg)
    again = evaluate_patch(ag, [(data, init)], gray, cfg)
    torch.cuda.synchronize()
    assert out.shape == (1, 4) and len(EVAL_KEYS) == 4 and out.device.type == "cuda" and not out.requires_grad
    assert torch.equal(out, again)
    assert _untouched(ag, snap)
    got = dict(zip(EVAL_KEYS, out[0].tolist()))
    params = load_case("walker_r2")[3]
    cpu = batch(z, 0, obs), initial(z, 0, spec)
    offset = (48, 24)
    ret_clean = irr.objective(spec, params, *cpu, ar.SEED, gray.cpu(), (1000, 1000))  # the window off the image
    ret_patched = irr.objective(spec, params, *cpu, ar.SEED, gray.cpu(), offset)
    _, kl, act = ar.objective(spec, params, *cpu, ar.SEED, gray.cpu(), offset)
    print(f"evaluate_patch {got}; oracle ret_clean {ret_clean:.6f}, ret_patched {ret_patched:.6f}, kl {kl:.5f}, "
          f"action {act:.6f}", flush=True)
    assert abs(got["ret_clean"] - ret_clean) <= sm.IMAG_ATOL + sm.IMAG_RTOL * abs(ret_clean)
    assert abs(got["ret_patched"] - ret_patched) <= sm.IMAG_ATOL + sm.IMAG_RTOL * abs(ret_patched)
    assert ret_clean != ret_patched
    assert abs(got["kl"] - kl) <= 6.4e-3 and abs(got["action"] - act) <= 0.05 * act
    assert kl > 0 and act > 0


def test_evaluate_patch_with_transforms_is_its_parts():
    """transforms=True over two batches equals, bit for bit, the same quantities assembled by hand: the seeded jitter
    and parameter draws, transform_rows, K.patch_apply_affine, agent.posterior and the loss objects."""
    from sdreamer import kernels as K
    from sdreamer.attack import (AdversarialPatch, PosteriorAttackLoss, eot_offsets, eot_ranges, eot_transforms,
                                 evaluate_patch, transform_rows)
    ag, z, spec, obs = build_agent("walker_r2")
    data, init = batch(z, 0, obs, DEV), initial(z, 0, spec, DEV)
    u8 = {**data, "image": torch.from_numpy(z["u0_in_image"]).to(DEV)}
    batches = [(data, init), (u8, init)]
    cfg = _cfg(eot_translations=2, max_jitter=3, **RANGES)
    g = torch.Generator().manual_seed(5)
    patch = AdversarialPatch((64, 64), 3, (16, 16), ar.PLACEMENT, device=DEV,
                             init=torch.rand(16, 16, 3, generator=g))
    held_out = 4242
    out = evaluate_patch(ag, batches, patch, cfg, seed=held_out, transforms=True)
    same = evaluate_patch(ag, batches, patch.patch.clone(), cfg, seed=held_out, transforms=True)  # the tensor form
    other = evaluate_patch(ag, batches, patch, cfg, seed=held_out + 1, transforms=True)
    plain = evaluate_patch(ag, batches, patch, cfg)
    B, T, H, W, C = data["image"].shape
    gen = torch.Generator().manual_seed(held_out)
    loss = PosteriorAttackLoss(1.0, 1.0, 0.0)
    want = torch.zeros(2, 4, device=DEV)
    with torch.no_grad():
        for j, (d, ini) in enumerate(batches):
            offs = eot_offsets((48, 24), B * T, 1, gen, 3)[B * T:]
            rows = transform_rows(offs, eot_transforms(B * T, 1, gen, *eot_ranges(cfg))[B * T:], (16, 16)).to(DEV)
            assert int((offs - torch.tensor([48, 24])).abs().max()) in (1, 2, 3)
            img, _ = K.patch_apply_affine(d["image"].reshape(-1, H, W, C).contiguous(), patch.patch, rows)
            post = ag.posterior(d, ini, seed=ar.SEED + j)
            adv = ag.posterior({**d, "image": img.view(B, T, H, W, C)}, ini, seed=ar.SEED + j)
            _, terms = loss(ag, loss.clean(ag, post), *adv)
            want[j, 0] = ag.imagined_return(post[0], post[1], None, seed=ar.SEED + j).mean()
            want[j, 1] = ag.imagined_return(adv[0], adv[1], None, seed=ar.SEED + j).mean()
            want[j, 2], want[j, 3] = terms["kl"], terms["action"]
    torch.cuda.synchronize()
    assert torch.equal(out, want) and torch.equal(out, same)
    assert torch.equal(out[:, 0], other[:, 0]) and not torch.equal(out[:, 1:], other[:, 1:])  # another seed, other draws
    assert torch.equal(out[:, 0], plain[:, 0]) and not torch.equal(out[:, 1:], plain[:, 1:])
    assert bool(torch.isfinite(out).all()) and float(out[:, 2].min()) > 0


def _act_case(B=4):
    from sdreamer.attack import AdversarialPatch
    ag, z, spec, obs_shapes = build_agent("walker_r2")
    obs, state = _inputs(spec, obs_shapes, B, int(z["meta_A"]), False, 9)
    obs = {k: v.to(DEV) for k, v in obs.items()}
    state = {k: v.to(DEV) for k, v in state.items()}
    g = torch.Generator().manual_seed(2)
    patch = AdversarialPatch((64, 64), 3, (16, 16), "bottom_center", device=DEV, init=torch.rand(16, 16, 3, generator=g))
    return ag, obs, state, patch


def _same(a, b):
    return torch.equal(a[0], b[0]) and all(torch.equal(a[1][k], b[1][k]) for k in b[1])


def test_patched_act_is_act_on_the_composited_observation():
    from sdreamer import kernels as K
    from sdreamer.attack import patched_act
    ag, obs, state, patch = _act_case()
    host = K.u8_to_f32(obs["image"]).cpu()
    for offsets in (None, [[10, -5], [-3, 30], [48, 24], [60, 60]]):
        pasted = host.clone()
        for n in range(host.shape[0]):
            oy, ox = (48, 24) if offsets is None else offsets[n]
            y0, y1, x0, x1 = max(oy, 0), min(oy + 16, 64), max(ox, 0), min(ox + 16, 64)
            pasted[n, y0:y1, x0:x1] = patch.patch.cpu()[y0 - oy:y1 - oy, x0 - ox:x1 - ox]
        offs = None if offsets is None else torch.tensor(offsets, dtype=torch.int32, device=DEV)
        for ev in (True, False):
            got = patched_act(ag, patch, obs, state, eval=ev, seed=77, step=3, offsets=offs)
            want = ag.act({**obs, "image": pasted.to(DEV)}, state, eval=ev, seed=77, step=3)
            clean = ag.act(obs, state, eval=ev, seed=77, step=3)
            assert _same(got, want), (offsets, ev)
            assert not torch.equal(got[0], clean[0])  # (the step's deter does not depend on the observation)
    # resampled: an identity row is the plain composite, a turned and re-lit patch is not
    from sdreamer.attack import transform_rows
    ident = transform_rows([[48, 24]] * 4, [[1.0, 0.0, 1.0, 0.0]] * 4, (16, 16)).to(DEV)
    turned = transform_rows([[48, 24]] * 4, [[1.2, 0.3, 1.1, 0.05]] * 4, (16, 16)).to(DEV)
    base = patched_act(ag, patch, obs, state, eval=True, seed=77)
    assert _same(patched_act(ag, patch, obs, state, eval=True, seed=77, transforms=ident), base)
    assert not torch.equal(patched_act(ag, patch, obs, state, eval=True, seed=77, transforms=turned)[0], base[0])


@pytest.mark.parametrize("resampled", [False, True], ids=["plain", "resampled"])
def test_patched_policy_graph_equals_patched_act_and_sees_a_stepped_patch(resampled):
    from sdreamer.attack import AdversarialPatch, patched_act, patched_policy_graph, transform_rows
    B = 4
    ag, obs, state, patch = _act_case(B)
    rows = transform_rows([[48, 24]] * B, [[1.2, 0.3, 1.1, 0.05]] * B, (16, 16)).to(DEV) if resampled else None
    policy = patched_policy_graph(ag, patch, B, obs, transforms=rows)
    base = ag._seed_base + 7
    st_g, st_e = dict(state), dict(state)
    for k in range(3):
        a_g, st_g = policy(obs, st_g)
        a_g, st_g = a_g.clone(), {n: v.clone() for n, v in st_g.items()}
        a_e, st_e = patched_act(ag, patch, obs, st_e, seed=base + k, step=0, transforms=rows)
        assert _same((a_g, st_g), (a_e, st_e)), k
    old = AdversarialPatch((64, 64), 3, (16, 16), "bottom_center", device=DEV, init=patch.patch)
    patch.step(torch.randn(16, 16, 3, generator=torch.Generator().manual_seed(1)).to(DEV))
    assert not torch.equal(old.patch, patch.patch)
    a_g, st_g2 = policy(obs, st_g)
    new = patched_act(ag, patch, obs, st_e, seed=base + 3, step=0, transforms=rows)
    stale = patched_act(ag, old, obs, st_e, seed=base + 3, step=0, transforms=rows)
    assert _same((a_g, st_g2), new)
    assert not torch.equal(a_g, stale[0])
