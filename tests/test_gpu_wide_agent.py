"""An agent whose conv encoder is wider than 128 channels, end to end: dmc/cnn with model.depth=33 (stages 66 / 99 /
132 / 132) at B2 x T4 x H3 against oracle/ref_cpu.OracleAgent in float64 (tests/wide_agent_models.py; the seed's
input condition is enforced by tests/test_wide_agent_cpu.py), and the reference's own width, model.depth=77.

Two update()s: posterior and imagined indices exact, world-model losses at 1e-4 relative; every encoder parameter
gradient of one _cal_grad within 2e-3 relative + 1e-4 of the tensor's max (test_cal_grad_matches_reference's bound);
the graphed update equal to the eager one bit for bit; observation_grad finite and equal across two calls; act and
policy_graph; state_dict in the reference layout; checkpoint save -> load -> one more update equal to the uninterrupted
run bit for bit. Before the wide row kernels existed, the first forward of this agent raised NativeError.
"""
import numpy as np
import pytest
import torch

import wide_agent_models as wa

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = wa.SEED


def _update(ag, u, seed=None):
    data, init = wa.product_batch(S, u % wa.UPDATES)
    out = ag.update_batch(data, init, wa.noise_seed(S, u) if seed is None else seed)
    torch.cuda.synchronize()
    return out


def _imag_idx(ag, spec):
    f = ag._last["imag_feat_tm"].detach().transpose(0, 1).cpu().numpy()  # (N, H + 1, F)
    return f[..., :spec.SK].reshape(f.shape[0], f.shape[1], spec.S, spec.K).argmax(-1)


@pytest.fixture(scope="module")
def eager_run():
    """two eager updates of the product, what each left behind, and the agent after them"""
    spec, _ = wa.spec_params(S)
    ag = wa.build_product(S)
    ag.use_graphs = False
    outs = []
    for u in range(wa.UPDATES):
        (ps, pd), mets = _update(ag, u)
        outs.append(dict(post_idx=ps.argmax(-1).cpu().numpy(), imag_idx=_imag_idx(ag, spec),
                         losses={k: float(mets[f"loss/{k}"]) for k in wa.WM_KEYS}, deter=pd.clone()))
    return ag, outs


def test_wide_stages_run_the_wide_kernels():
    from wide_conv_models import Launches
    ag = wa.build_product(S)
    ag.use_graphs = False
    with Launches() as rec:
        _update(ag, 0)
    # stages 3 and 4 (132 channels) on the wide row kernels, their three contractions with a side above 128 on the
    # wide arms (stage 3's two, stage 4's two, and none for 66 -> 99); stages 1 and 2 where they were
    assert rec.count("sd_pool_rms_wide_fwd") == 2 and rec.count("sd_pool_rms_wide_bwd") == 2
    assert rec.count("sd_conv2d_wgrad_wide3") == 2 and rec.count("sd_conv2d_dgrad_wide3") == 2


def test_two_updates_match_the_float64_oracle(eager_run):
    _, outs = eager_run
    ref = wa.run_oracle(S, torch.float64)
    for u, (got, want) in enumerate(zip(outs, ref)):
        assert np.array_equal(got["post_idx"], want["post_idx"]), f"update {u}: posterior indices"
        assert np.array_equal(got["imag_idx"], want["imag_idx"]), f"update {u}: imagined indices"
        rel = {k: abs(got["losses"][k] - want["losses"][k]) / max(abs(want["losses"][k]), 1e-6) for k in wa.WM_KEYS}
        print(f"update {u}: world-model loss relative errors", {k: f"{v:.2g}" for k, v in rel.items()})
        assert all(v <= 1e-4 for v in rel.values()), rel


def test_encoder_gradients_match_the_float64_oracle():
    ag = wa.build_product(S)
    ag.use_graphs = False
    data, init = wa.product_batch(S, 0)
    pre = ag.preprocess(dict(data), enc_input=True)
    ag._update_slow_target()
    ag._optimizer.zero_grad()
    ag._cal_grad(pre, init, wa.noise_seed(S, 0), 0)
    torch.cuda.synchronize()
    ref = wa.oracle_encoder_grads(S)
    named = dict(ag.named_parameters())
    assert len(ref) == 12, sorted(ref)  # four stages: conv weight, conv bias, norm weight
    bad, worst = [], (0.0, None)
    for k, r in ref.items():
        g = ag.to_ref_layout(named[k], named[k].grad).double().cpu().numpy()
        assert g.shape == r.shape, k
        scale = np.abs(r).max()
        ratio = float((np.abs(g - r) / (2e-3 * np.abs(r) + 1e-4 * scale + 1e-12)).max())
        if not ratio <= 1.0:
            bad.append((k, ratio))
        worst = max(worst, (ratio, k))
    print("worst fraction of an encoder gradient bound used", worst)
    assert not bad, bad


def test_graphed_update_equals_eager(eager_run):
    eager, _ = eager_run
    spec, _ = wa.spec_params(S)
    ag = wa.build_product(S)
    assert ag.use_graphs
    for u in range(wa.UPDATES):  # the eager warm-up updates
        _update(ag, u)
    s1, s2 = eager.state_dict(), ag.state_dict()
    assert not [k for k in s1 if not torch.equal(s1[k], s2[k])]
    (_, pd_g), m_g = _update(ag, 2, seed=4242)  # captured and replayed
    assert ag._graph is not None
    (_, pd_e), m_e = _update(eager, 2, seed=4242)
    assert torch.equal(pd_g, pd_e)
    assert {k: float(m_g[f"loss/{k}"]) for k in wa.WM_KEYS} == {k: float(m_e[f"loss/{k}"]) for k in wa.WM_KEYS}
    s1, s2 = eager.state_dict(), ag.state_dict()
    assert not [k for k in s1 if not torch.equal(s1[k], s2[k])]


def test_observation_grad_is_finite_and_repeatable(eager_run):
    ag, _ = eager_run
    data, init = wa.product_batch(S, 0)

    def loss_fn(stoch, deter, logit):
        return deter.square().mean() + logit.square().mean()

    l1, g1 = ag.observation_grad(data, init, loss_fn, seed=5)
    l2, g2 = ag.observation_grad(data, init, loss_fn, seed=5)
    torch.cuda.synchronize()
    assert g1.shape == (wa.B, wa.T, 64, 64, 3) and g1.isfinite().all() and g1.abs().max() > 0
    assert torch.equal(g1, g2) and torch.equal(l1, l2)


def test_act_and_policy_graph(eager_run):
    ag, _ = eager_run
    obs = {"image": torch.from_numpy(wa.inputs(S, 0)[0]["image"][:, 0]).to(DEV),
           "is_first": torch.ones(wa.B, dtype=torch.bool, device=DEV)}
    st = ag.get_initial_state(wa.B)
    policy = ag.policy_graph(wa.B, obs)
    base = ag._seed_base + 7
    st_g, st_e = dict(st), dict(st)
    for k in range(3):
        a_g, st_g = policy(obs, st_g)
        a_g, st_g = a_g.clone(), {n: v.clone() for n, v in st_g.items()}
        a_e, st_e = ag.act(obs, st_e, seed=base + k, step=0)
        assert a_e.shape == (wa.B, wa.A) and a_e.isfinite().all()
        assert torch.equal(a_g, a_e), k
        for n in st_e:
            assert torch.equal(st_g[n], st_e[n]), (k, n)


def test_state_dict_and_checkpoint_resume(eager_run, tmp_path):
    from sdreamer.checkpoint import load_checkpoint, save_checkpoint
    ag, _ = eager_run
    spec, _ = wa.spec_params(S)
    sd = ag.state_dict()
    for k, shape in spec.shapes.items():  # the reference's names and layouts (conv: (Co, Ci, k, k))
        assert k in sd and tuple(sd[k].shape) == tuple(shape), k
    assert tuple(sd["encoder.encoders.0.layers.8.weight"].shape) == (132, 99, 5, 5)
    path = save_checkpoint(ag, str(tmp_path / "latest.pt"))
    ag2 = wa.build_product(S + 1)  # other weights, then the checkpoint
    ag2.use_graphs = False
    load_checkpoint(ag2, path)
    assert ag2._updates == ag._updates
    r1, r2 = _update(ag, 0, seed=777), _update(ag2, 0, seed=777)
    assert torch.equal(r1[0][1], r2[0][1]) and float(r1[1]["opt/loss"]) == float(r2[1]["opt/loss"])
    s1, s2 = ag.state_dict(), ag2.state_dict()
    assert not [k for k in s1 if not torch.equal(s1[k], s2[k])]


def test_reference_width_depth_77_updates():
    """model.depth=77 (stages 154 / 231 / 308 / 308, the reference's h3_wider_cnn): one update at B1 x T2, finite"""
    from sdreamer.config import load_config
    assert int(load_config("dmc/wider_cnn").model.depth) == 77
    ag = wa.build_product(S, depth=77)
    ag.use_graphs = False
    assert ag.encoder.out_dim == 4928
    data, init = wa.product_batch(S, 0)
    data = {k: v[:1, :2].contiguous() for k, v in data.items()}
    (ps, pd), mets = ag.update_batch(data, ag.rssm.initial(1), 11)
    torch.cuda.synchronize()
    assert all(np.isfinite(float(v)) for k, v in mets.items() if k.startswith("loss/")), mets
    assert pd.isfinite().all()


def test_depth_77_encoder_matches_the_reference_pin():
    """The product's conv encoder at the reference's width against the reference's own ConvEncoder (the fixture
    tests/golden/encoder_wide_h3.npz, tests/wide_golden_io.py): outputs within 1e-4 + 1e-4 |ref|; under the probe loss
    every gradient's norm within 2e-4 and its sampled elements within 2e-3 relative + 1e-4 of the largest sampled |g|
    (test_gpu_imgrad.py's bounds) of the reference's f32 gradient, or of the float64 restatement's where the
    reference's own f32 is farther than that from exact arithmetic (test_wide_golden_cpu.py has the figures)."""
    import wide_golden_io as wg
    z = np.load(wg.FIXTURE)
    ag = wa.build_product(S, depth=77)
    missing, unexpected = ag.load_state_dict({k: torch.from_numpy(v) for k, v in wg.params().items()}, strict=False)
    assert not unexpected and not [m for m in missing if m.startswith(wg.PREFIX)]
    ag._optimizer.zero_grad()
    out = ag.encoder({"image": torch.from_numpy(wg.frames()).to(DEV)}).reshape(wg.FRAMES, -1)
    (out * torch.from_numpy(wg.probe()).to(DEV)).sum().backward()
    torch.cuda.synchronize()
    named = dict(ag.named_parameters())
    grads = {k: ag.to_ref_layout(named[k], named[k].grad).double().cpu().numpy() for k in wg.shapes()}
    do, per = wg.distance(out.detach().cpu().numpy(), grads, z)
    o64, g64 = wg.restate(torch.float64)
    do64, per64 = wg.distance(out.detach().cpu().numpy(), grads, wg.summarise(o64, g64))
    print("output: fraction of the bound vs the reference", do, "vs float64", do64)
    print({k[len(wg.PREFIX):]: (round(max(per[k]), 3), round(max(per64[k]), 3)) for k in per})
    assert do <= 1.0
    bad = [(k, per[k], per64[k]) for k in per if min(max(per[k]), max(per64[k])) > 1.0]
    assert not bad, bad
