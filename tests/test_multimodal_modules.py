"""Text-conditioned encoder modules (sdreamer/multimodal.py), host side: the reference's parameter names and shapes,
its initialisers, and the text schedule (a draw every 64 training forwards, the first text in eval, a clear error
without features). Nothing here launches a kernel."""
import random
import types

import numpy as np
import pytest
import torch


def _cnn_cfg():
    return types.SimpleNamespace(depth=16, mults=[2, 3, 4, 4], kernel_size=5, norm=True, act="SiLU")


def _mm(**kw):
    from sdreamer.multimodal import MultimodalEncoder
    return MultimodalEncoder(_cnn_cfg(), (64, 64, 3), **kw)


# the reference's state_dict at walker 64 x 64 x 3 (E = 1024), without the frozen CLIP weights
def _expected(prefix_visual=True):
    exp = {
        "text_context_encoder.attn_pool.weight": (1, 512), "text_context_encoder.attn_pool.bias": (1,),
        "text_context_encoder.proj.weight": (256, 512), "text_context_encoder.proj.bias": (256,),
        "text_gate.text_proj.0.weight": (1024, 256), "text_gate.text_proj.0.bias": (1024,),
        "text_gate.text_proj.2.weight": (1024, 1024), "text_gate.text_proj.2.bias": (1024,),
        "text_gate.gate_net.0.weight": (1024, 2048), "text_gate.gate_net.0.bias": (1024,),
        "text_gate.gate_net.2.weight": (1024, 1024), "text_gate.gate_net.2.bias": (1024,),
    }
    ci = 3
    for i, c in enumerate((32, 48, 64, 64)):
        if prefix_visual:
            exp[f"visual_encoder.convs.{i}.weight"] = (c, ci, 5, 5)
            exp[f"visual_encoder.convs.{i}.bias"] = (c,)
            exp[f"visual_encoder.norms.{i}.weight"] = (c,)
            exp[f"visual_encoder.films.{i}.net.0.weight"] = (2 * c, 256)
            exp[f"visual_encoder.films.{i}.net.0.bias"] = (2 * c,)
            exp[f"visual_encoder.films.{i}.net.2.weight"] = (2 * c, 2 * c)
            exp[f"visual_encoder.films.{i}.net.2.bias"] = (2 * c,)
        else:
            exp[f"conv_encoder.layers.{4 * i}.weight"] = (c, ci, 5, 5)
            exp[f"conv_encoder.layers.{4 * i}.bias"] = (c,)
            exp[f"conv_encoder.layers.{4 * i + 2}.weight"] = (c,)
        ci = c
    return exp


def test_multimodal_state_dict_matches_reference_layout():
    enc = _mm()
    sd = enc.state_dict()
    assert {k: tuple(v.shape) for k, v in sd.items()} == _expected()
    assert enc.out_dim == 1024
    # conv weights convert like networks.Conv2d: a reference-layout dict loads back to the same values
    enc2 = _mm()
    enc2.load_state_dict(sd)
    for (k, a), b in zip(enc.state_dict().items(), enc2.state_dict().values()):
        assert torch.equal(a, b), k


def test_gate_only_state_dict_matches_reference_layout():
    from sdreamer.multimodal import GateOnlyEncoder
    enc = GateOnlyEncoder(_cnn_cfg(), (64, 64, 3))
    assert {k: tuple(v.shape) for k, v in enc.state_dict().items()} == _expected(prefix_visual=False)


def test_film_only_has_no_gate():
    enc = _mm(use_text_gate=False)
    assert not any(k.startswith("text_gate.") for k in enc.state_dict())


def test_mlp_projector_layout_and_eps():
    from sdreamer.multimodal import MLPProjector
    prj = MLPProjector(2560, 1024)
    assert {k: tuple(v.shape) for k, v in prj.state_dict().items()} == {
        "fc1.weight": (1024, 2560), "norm.weight": (1024,), "fc2.weight": (1024, 1024)}
    assert prj.EPS == float(torch.finfo(torch.float32).eps)  # nn.RMSNorm(eps=None) in an f32 run, not kernels.EPS


def test_initialisers_follow_reference():
    torch.manual_seed(0)
    enc = _mm(gate_init_bias=-3.0)
    for film in enc.visual_encoder.films:
        assert not film.net[2].weight.any() and not film.net[2].bias.any()  # identity modulation at init
        assert not film.net[0].bias.any()
    g = enc.text_gate.gate_net
    assert not g[2].weight.any() and torch.all(g[2].bias == -3.0)
    # xavier-uniform: U(-a, a), a = sqrt(6 / (fan_in + fan_out)); std a / sqrt(3)
    for lin in (enc.text_gate.text_proj[0], enc.text_gate.text_proj[2], g[0], enc.visual_encoder.films[1].net[0],
                enc.text_context_encoder.proj):
        o, i = lin.weight.shape
        a = (6.0 / (i + o)) ** 0.5
        w = lin.weight.detach()
        assert w.abs().max().item() <= a
        assert abs(w.std().item() / (a / 3 ** 0.5) - 1) < 0.05, (o, i)
        assert w.abs().max().item() > 0.95 * a  # uniform up to the bound, not a truncated normal
        assert not lin.bias.any()
    # the text front end never trains (the reference detaches the context before the loss)
    assert not any(p.requires_grad for p in enc.text_context_encoder.parameters())


def _feats(n_texts):
    g = torch.Generator().manual_seed(5)
    return [torch.randn(5 + i, 512, generator=g).numpy() for i in range(n_texts)]


def test_missing_text_features_raise():
    enc = _mm()
    with pytest.raises(ValueError, match="text features"):
        enc.set_task_name("walker_walk")
    with pytest.raises(ValueError, match="text features"):
        enc.text_context(2, "cpu")
    with pytest.raises(ValueError):
        enc.set_text_features(["a"], [np.zeros((3, 100), np.float32)])  # wrong clip_dim
    with pytest.raises(ValueError):
        enc.set_text_features(["a", "b"], [np.zeros((3, 512), np.float32)])


def test_text_schedule_resamples_every_64_training_forwards():
    n, seed = 7, 11
    enc = _mm(seed_base=seed)
    enc.set_text_features([f"t{i}" for i in range(n)], _feats(n))
    enc.set_task_name("walker_walk")
    draw = [random.Random(seed * 1000003 + r).randrange(n) for r in range(3)]  # the schedule restated
    seen = {}
    enc.train()
    for fwd in range(129):
        seen[fwd] = enc._next_text()
    assert seen[0] == draw[0] and seen[63] == draw[0]
    assert seen[64] == draw[1] and seen[127] == draw[1]
    assert seen[128] == draw[2]
    assert all(seen[f] == draw[f // 64] for f in range(129))
    # a run repeats
    enc2 = _mm(seed_base=seed)
    enc2.set_text_features([f"t{i}" for i in range(n)], _feats(n))
    assert enc2._next_text() == draw[0]
    # eval: the first text, and no forward is counted
    enc.eval()
    count = enc._forward_count
    assert enc._next_text() == 0 and enc._forward_count == count


def test_text_features_npz_round_trip(tmp_path):
    feats = _feats(2)
    path = tmp_path / "texts.npz"
    np.savez(path, texts=np.array(["first", "second"]), feat_0=feats[0], feat_1=feats[1])
    enc = _mm()
    enc.load_text_features(str(path))
    assert enc._texts == ["first", "second"]
    assert torch.equal(enc._feats[1], torch.from_numpy(feats[1]))


@pytest.mark.parametrize("name", ["dmc/multimodal", "dmc/distractor_multimodal"])
def test_multimodal_configs_load(name):
    from sdreamer.config import load_config
    cfg = load_config(name)
    assert cfg.model.use_multimodal_encoder is True
    mc = cfg.model.multimodal_encoder
    assert mc.use_text_gate is True and mc.gate_init_bias == -3 and mc.text_context_dim == 256
    assert mc.text_features is None  # the frozen token features are user data (null: agent.set_text_features)
    assert cfg.model.loss_scales.rew == 1.0  # the base table survives the case's partial override
    assert bool(cfg.model.r2dreamer.aug.enabled) == (name == "dmc/distractor_multimodal")
