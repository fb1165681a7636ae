"""Dreamer with model.use_multimodal_encoder=True on the MI355X: the update through the phase schedule and the HIP
graphs (graph replay == eager bit for bit, with a text switch after capture), the gated embed in act / policy_graph,
the checkpoint layout, the stated limits. Batches are the walker_r2 fixture's inputs (B2 T6 H4)."""
import copy

import numpy as np
import pytest
import torch

from golden_io import batch, initial, load_case
from sdreamer.config import load_config
from test_gpu_dreamer import _Sp, _Spaces

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FRONT = ["encoder.text_context_encoder.attn_pool.weight", "encoder.text_context_encoder.attn_pool.bias",
         "encoder.text_context_encoder.proj.weight", "encoder.text_context_encoder.proj.bias"]
VARIANTS = {"mm": [], "filmonly": ["model.multimodal_encoder.use_text_gate=False"],
            "gateonly": ["model.ablation_encoder_type=gate_only"]}


def _feats():
    g = torch.Generator().manual_seed(3)
    return ["a walker", "two legs move right"], [torch.randn(n, 512, generator=g) for n in (7, 12)]


def _agent(variant="mm", extra=(), features=True, **kw):
    from sdreamer.dreamer import Dreamer
    z, _, spec, _, obs = load_case("walker_r2")
    cfg = load_config("dmc/multimodal", ["device=cuda:0", "model.compile=False",
                                         f"model.imag_horizon={int(z['meta_H'])}"] + VARIANTS[variant] + list(extra))
    torch.manual_seed(0)
    ag = Dreamer(copy.deepcopy(cfg.model), _Spaces({k: _Sp(v) for k, v in obs.items()}), _Sp((int(z["meta_A"]),)), **kw)
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():  # the zero-initialised FiLM / gate layers made dense, so the text conditions the update
        for n, p in ag.named_parameters():
            if n.startswith("encoder.") and (".films." in n and ".net.2." in n or n.endswith("gate_net.2.weight")):
                p.copy_((0.3 * torch.randn(p.shape, generator=g) / max(p.shape[-1], 1) ** 0.5).to(p.device))
    if features:
        ag.set_text_features(*_feats())
        ag.set_task_name("walker_walk")
    return ag, z, spec, obs


def _run(variant, graphs):
    ag, z, spec, obs = _agent(variant)
    ag.use_graphs = graphs
    sd0 = {k: v.detach().clone() for k, v in ag.state_dict().items()}
    out, texts = [], []
    for u in range(5):
        if u == 3:  # a text switch between updates 3 and 4, after the capture (updates 1-2 eager, 3 captures)
            ag.encoder._text_index = 1 - ag.encoder._text_index
        (ps, pd), mets = ag.update_batch(batch(z, u % 2, obs, DEV), initial(z, u % 2, spec, DEV), 500 + u)
        texts.append(ag.encoder._cached_index)
        out.append(({k: float(v) for k, v in mets.items()}, pd.detach().clone(), ps.argmax(-1).clone()))
    return ag, sd0, out, texts


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_graph_replay_matches_eager_with_text_switch(variant):
    (age, sd0, e, te), (agg, _, g, tg) = _run(variant, False), _run(variant, True)
    assert agg._graph is not None and age._graph is None
    assert te == tg and te[2] != te[3], te  # the switch happened, between two replays
    for u in range(5):
        assert e[u][0].keys() == g[u][0].keys()
        diff = {k: (e[u][0][k], g[u][0][k]) for k in e[u][0] if e[u][0][k] != g[u][0][k]}
        assert not diff, (u, diff)
        assert torch.equal(e[u][1], g[u][1]) and torch.equal(e[u][2], g[u][2]), u
        assert all(np.isfinite(v) for v in e[u][0].values()), u
    if variant != "filmonly":
        assert 0 < e[0][0]["encoder/text_gate_mean"] < 1 and e[0][0]["encoder/text_gate_std"] > 0
    sde, sdg = age.state_dict(), agg.state_dict()
    bad = [k for k in sde if not torch.equal(sde[k], sdg[k])]
    assert not bad, bad[:8]
    for k in FRONT:  # the text front end never moves
        assert torch.equal(sde[k], sd0[k]), k
    moved = [k for k in sde if k.startswith("encoder.") and k not in FRONT and not torch.equal(sde[k], sd0[k])]
    still = [k for k in sde if k.startswith("encoder.") and k not in FRONT and k not in moved]
    assert not still, f"encoder tensors without an update: {still}"
    assert all(k.split("encoder.")[1] not in n for n in age._named_params for k in FRONT)


def test_text_changes_the_update():
    """same batch, same seed, the other text: the posterior differs (the context reaches the scan's input)"""
    res = []
    for idx in (0, 1):
        ag, z, spec, obs = _agent("mm")
        ag.use_graphs = False
        ag.encoder.text_context(2, ag.device, force_index=idx)
        ag.encoder._text_index, ag.encoder._forward_count = idx, 1
        (ps, pd), _ = ag.update_batch(batch(z, 0, obs, DEV), initial(z, 0, spec, DEV), 500)
        res.append(pd.clone())
    assert not torch.equal(res[0], res[1])


def _act_inputs(ag, B, seed):
    g = torch.Generator().manual_seed(seed)
    obs = {"image": torch.randint(0, 256, (B, 64, 64, 3), dtype=torch.uint8, generator=g).to(DEV),
           "is_first": torch.tensor([i % 3 == 0 for i in range(B)]).to(DEV)}
    st = ag.get_initial_state(B)
    st["deter"] = (0.3 * torch.randn(st["deter"].shape, generator=g)).to(DEV)
    return obs, st


@pytest.mark.parametrize("variant", list(VARIANTS))
def test_act_uses_gated_embed_and_policy_graph_equals_act(variant):
    from sdreamer.rssm import STREAM_POLICY
    ag, z, spec, _ = _agent(variant)
    B = 3
    obs, st = _act_inputs(ag, B, 4)
    a, s = ag.act(obs, st, eval=True, seed=321, step=2)
    with torch.no_grad():  # the encoder + gate forward at T = 1, restated
        ctx = ag.encoder.act_context(B, ag.device, eval=True)
        out = ag.encoder({"image": ag.preprocess(dict(obs))["image"]}, reuse_text_context=ctx)
        visual, embed = out if isinstance(out, tuple) else (out, out)
        stoch, deter, _ = ag.rssm.obs_step(st["stoch"], st["deter"], st["prev_action"], embed, obs["is_first"],
                                           seed=321, step=2, stream_id=STREAM_POLICY)
    assert torch.equal(s["stoch"], stoch) and torch.equal(s["deter"], deter)
    if variant != "filmonly":
        assert not torch.equal(visual, embed)
    assert ag.encoder._act["cached"] == 0 and ag.encoder._ctx is None  # act never touches the update's buffer
    policy = ag.policy_graph(B, obs)
    base = ag._seed_base + 7
    st_g, st_e = dict(st), dict(st)
    for k in range(3):
        a_g, st_g = policy(obs, st_g)
        a_g, st_g = a_g.clone(), {n: v.clone() for n, v in st_g.items()}
        a_e, st_e = ag.act(obs, st_e, seed=base + k, step=0)
        assert torch.equal(a_g, a_e), k
        for n in st_e:
            assert torch.equal(st_g[n], st_e[n]), (k, n)


def test_checkpoint_round_trip(tmp_path):
    from sdreamer.checkpoint import load_checkpoint, save_checkpoint
    ag, z, spec, obs = _agent("mm")
    ag.use_graphs = False
    for u in range(2):
        ag.update_batch(batch(z, u, obs, DEV), initial(z, u, spec, DEV), 500 + u)
    sd = ag.state_dict()
    assert all(("_frozen_" + k) in sd for k in FRONT) and "_frozen_encoder.text_gate.gate_net.2.bias" in sd
    assert not any("_text_model" in k for k in sd)
    # the optimizer state keeps the reference's parameter order: the four front-end tensors hold slots (the
    # reference lists them) and no state entry (it never gives them a gradient)
    names = [f"{m}.{pn}" for m, mod in (("rssm", ag.rssm), ("actor", ag.actor), ("value", ag.value),
                                        ("reward", ag.reward), ("cont", ag.cont), ("encoder", ag.encoder),
                                        ("projector", ag.prj)) for pn, _ in mod.named_parameters()]  # dreamer.py:199-206
    osd = ag._optimizer.state_dict()
    slots = [names.index(k) for k in FRONT]
    assert osd["param_groups"][0]["params"] == list(range(len(names))) and len(names) == len(ag._named_params) + 4
    assert set(osd["state"]) == set(range(len(names))) - set(slots)
    i_prj = names.index("projector.fc1.weight")  # a tensor behind the four slots keeps the reference's index
    assert tuple(osd["state"][i_prj]["exp_avg"].shape) == tuple(ag.prj.fc1.weight.shape)
    path = str(tmp_path / "latest.pt")
    save_checkpoint(ag, path)
    ag2, *_ = _agent("mm")
    ag2.use_graphs = False
    load_checkpoint(ag2, path)
    # a reference checkpoint also carries the frozen CLIP weights: skipped on load
    extra = {k: v.clone() for k, v in sd.items()}
    extra["encoder.text_context_encoder._text_model.text_model.embeddings.token_embedding.weight"] = torch.zeros(4, 4)
    extra["_frozen_encoder.text_context_encoder._text_model.text_model.final_layer_norm.bias"] = torch.zeros(4)
    ag2.load_state_dict(extra)
    assert ag2.encoder.text_schedule_state() == ag.encoder.text_schedule_state()  # resumed with the checkpoint
    r1 = ag.update_batch(batch(z, 0, obs, DEV), initial(z, 0, spec, DEV), 777)
    r2 = ag2.update_batch(batch(z, 0, obs, DEV), initial(z, 0, spec, DEV), 777)
    assert torch.equal(r1[0][1], r2[0][1]) and float(r1[1]["opt/loss"]) == float(r2[1]["opt/loss"])
    s1, s2 = ag.state_dict(), ag2.state_dict()
    assert not [k for k in s1 if not torch.equal(s1[k], s2[k])]


def test_stated_limits():
    with pytest.raises(NotImplementedError, match="dreamerpro"):
        _agent("mm", extra=["model.rep_loss=dreamerpro"], features=False)
    with pytest.raises(NotImplementedError, match="more than one GPU"):
        _agent("mm", features=False, rank=0, world=2)
    ag, z, spec, obs = _agent("mm", features=False)
    with pytest.raises(ValueError, match="text features"):
        ag.set_task_name("walker_walk")
    with pytest.raises(ValueError, match="text features"):
        ag.update_batch(batch(z, 0, obs, DEV), initial(z, 0, spec, DEV), 1)
