"""d loss / d observation through the encoder and the RSSM posterior (Dreamer.posterior(with_grad=True),
Dreamer.observation_grad) against the reference's image gradient (tests/golden/walker_r2_imgrad.npz), the multimodal
encoder's against its float64 restatement, and the update path left as it was."""
import numpy as np
import pytest
import torch

import imgrad_ref as ir
from golden_io import batch, initial
from test_gpu_dreamer import build_agent

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _probe(ag, R, keep):
    """the fixture's probe loss on the product's own kernels (prior, KL) with torch's reductions"""
    def loss_fn(post_stoch, post_deter, post_logit):
        keep["idx"] = post_stoch.detach().argmax(-1).cpu().numpy()
        dyn, rep = ag.rssm.kl_loss(post_logit, ag.rssm.prior(post_deter), 0.0)
        return ir.probe_loss_terms(dyn, rep, post_deter, R)
    return loss_fn


def _check(g, ref_norm, ref_s, what):
    """test_cal_grad_matches_reference's bounds: sampled elements within 2e-3 relative + 1e-4 of the largest sampled
    |g|, per-frame norms within 2e-4"""
    norms, elems = ir.sampled(g.detach().cpu().numpy())
    dn, de = ir.distance(norms, elems, ref_norm, ref_s)
    print(f"{what}: per-frame norm {dn / 2e-4:.4f} of its bound, sampled elements {de:.4f} of theirs", flush=True)
    assert dn <= 2e-4, (what, "norm", dn)
    assert de <= 1.0, (what, "element", de)


def test_observation_grad_matches_reference():
    """observation_grad on the walker_r2_imgrad inputs with the fixture's probe loss (mean dyn + mean rep without free
    bits + <post_deter, R>): posterior indices exact; per-frame norms within 2e-4 and the 4,096 sampled elements within
    2e-3 relative + 1e-4 of the largest sampled |g| of the reference's f32 gradient. The oracle's own f32 sits 3.6e-7
    (norms) and 0.0077 of the element bound from float64 on this gradient (tests/test_imgrad_attack_cpu.py), far
    below half of these bounds, so they hold against the reference's f32 values unchanged. Before the image gradient
    existed this raised NotImplementedError("input gradient through a channel-padded conv")."""
    from sdreamer import kernels as K
    ag, _, spec, obs = build_agent("walker_r2")
    z = ir.load_fixture()
    data, init = ir.fixture_inputs(z, obs, spec, DEV)
    R = torch.from_numpy(z["R"]).to(DEV)
    keep = {}
    before = K.DGRAD_POOL_CALLS
    loss, g = ag.observation_grad(data, init, _probe(ag, R, keep), seed=int(z["seed"]))
    torch.cuda.synchronize()
    assert K.DGRAD_POOL_CALLS == before + 1  # the first stage's input gradient came from the pooled-gradient kernel
    assert g.shape == data["image"].shape == (2, 6, 64, 64, 3)
    assert np.array_equal(keep["idx"], z["post_idx"])
    assert abs(float(loss) - float(z["loss"])) <= 1e-4 * abs(float(z["loss"]))
    _check(g, z["g_norm"], z["g_s"].astype(np.float64), "walker_r2 d loss / d image")
    # the same from uint8 frames, and bit for bit on repetition
    u8 = {**data, "image": torch.from_numpy(z["in_image"]).to(DEV)}
    _, g2 = ag.observation_grad(u8, init, _probe(ag, R, keep), seed=int(z["seed"]))
    assert torch.equal(g, g2)
    assert all(p.grad is None or not bool(p.grad.any()) for p in ag.parameters())


def test_posterior_without_grad_is_the_update_posterior():
    ag, z, spec, obs = build_agent("walker_r2")
    data, init = batch(z, 0, obs, DEV), initial(z, 0, spec, DEV)
    ps, pd, pl = ag.posterior(data, init, seed=int(z["u0_seed"]))
    assert not ps.requires_grad and not pl.requires_grad
    assert np.array_equal(ps.argmax(-1).cpu().numpy(), z["u0_post_idx"])
    with pytest.raises(ValueError):
        ag.posterior(data, init, with_grad=True)  # the image does not require grad


def test_update_path_is_unchanged():
    """An image that does not require grad: the first stage's backward issues no new launch (conv2d_dgrad_pool is
    never called during _cal_grad), and the parameter gradients of one _cal_grad are bit-identical whether or not
    posterior(with_grad=True) and its backward ran just before: nothing leaks into the gradient arena."""
    from sdreamer import kernels as K
    grads = []
    for attack_first in (False, True):
        ag, z, spec, obs = build_agent("walker_r2")
        ag.use_graphs = False
        data = ag.preprocess(batch(z, 0, obs, DEV))
        init = initial(z, 0, spec, DEV)
        ag._update_slow_target()
        ag._optimizer.zero_grad()
        clean = ag._grads_clean
        if attack_first:
            img = data["image"].clone().requires_grad_()
            before = K.DGRAD_POOL_CALLS
            ps, pd, pl = ag.posterior({**data, "image": img}, init, seed=7, with_grad=True)
            (pl.square().mean() + pd.sum()).backward()
            torch.cuda.synchronize()
            assert K.DGRAD_POOL_CALLS == before + 1 and bool(img.grad.abs().sum() > 0)
            assert ag._grads_clean == clean
            assert all(p.grad is None or not bool(p.grad.any()) for p in ag.parameters())
            from sdreamer import ops
            assert ops._GRAD_SINK is None  # the routing ended with the backward
        before = K.DGRAD_POOL_CALLS
        ag._cal_grad(data, init, 1000, 0)
        torch.cuda.synchronize()
        assert K.DGRAD_POOL_CALLS == before
        grads.append({k: p.grad.clone() for k, p in ag.named_parameters() if p.grad is not None})
    assert grads[0].keys() == grads[1].keys() and len(grads[0]) > 20
    for k in grads[0]:
        assert torch.equal(grads[0][k], grads[1][k]), k


def test_multimodal_observation_grad_matches_float64():
    """The same check with the FiLM encoder and the text gate (walker_mm_r2's weights and update-0 inputs, B2 T6, its
    text): against tests/mm_ref.py's float64 encoder (differentiable to the image) followed by the oracle's observe
    in float64 under autograd, on the same bounds; posterior indices exact (the fixture's own too)."""
    import mm_ref
    from oracle import ref_cpu
    from test_gpu_multimodal_update import OBS, _build
    ag, z, spec, shapes, params = _build("walker_mm_r2")
    B, T = int(z["meta_B"]), int(z["meta_T"])
    text = int(z["u0_text"])
    data, init = batch(z, 0, OBS, DEV), initial(z, 0, spec, DEV)
    seed = int(z["u0_seed"])
    R = ir.probe_R(B, T, spec.D)
    keep = {}
    loss, g = ag.observation_grad(data, init, _probe(ag, torch.from_numpy(R).to(DEV), keep), seed=seed,
                                  text_ctx=ag._posterior_text_ctx(B, text))
    torch.cuda.synchronize()
    assert np.array_equal(keep["idx"], z["u0_post_idx"])
    # float64 restatement on the CPU
    ref_cpu.DT = torch.float64
    try:
        P = {k: torch.from_numpy(v).double() for k, v in params.items()}
        Penc = {k[len("encoder."):]: v for k, v in P.items() if k.startswith("encoder.")}
        M = ref_cpu.Oracle(spec, P)
        cpu = batch(z, 0, OBS)
        img = cpu["image"].double().requires_grad_()
        _, gated, _, _ = mm_ref.encoder_ref(Penc, torch.from_numpy(z[f"feat_{text}"]), img, B, T, "mm", True)
        ini = tuple(t.double() for t in initial(z, 0, spec))
        ps, pd, pl = M.observe(gated.reshape(B, T, -1), cpu["action"].double(), ini, cpu["is_first"], seed)
        prior = M.img_logit(pd)
        rep = ref_cpu.kl_cat(pl, prior.detach()).sum(-1)
        dyn = ref_cpu.kl_cat(pl.detach(), prior).sum(-1)
        ref_loss = ir.probe_loss_terms(dyn, rep, pd, torch.from_numpy(R).double())
        ref_loss.backward()
    finally:
        ref_cpu.DT = torch.float32
    assert np.array_equal(ps.detach().argmax(-1).numpy(), keep["idx"])
    assert abs(float(loss) - float(ref_loss.detach())) <= 1e-4 * abs(float(ref_loss.detach()))
    _check(g, *ir.sampled(img.grad.numpy()), "walker_mm_r2 d loss / d image")
    assert all(p.grad is None or not bool(p.grad.any()) for p in ag.parameters())
