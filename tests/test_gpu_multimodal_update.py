"""The multimodal update against the reference's own Dreamer (tests/golden/walker_mm_*.npz, written by
gen_golden_mm.py): two update_batch calls forced onto the fixture's two texts, the gradients of one _cal_grad whose
text context differs per batch row, and the initialisers. Bounds are test_gpu_dreamer's (test_update_matches_reference,
test_cal_grad_matches_reference, test_weight_init_matches_reference), without their float64 fall-back; the fixtures'
batch seeds keep every categorical draw at least 2e-4 from a tie, so indices are compared exactly.

Worst fraction of a bound used per class, measured on the MI355X (bound_ratio, <= 1 passes; r2 / filmonly / gateonly):
  embeds + text context 0.19 / 0.22 / 0.13    post_deter 0.007 / 0.007 / 0.010    logits 0.026 / 0.028 / 0.025
  imagination 0.06 / 0.10 / 0.08    returns 0.002 / 0.001 / 0.001    world-model losses 0.002 / 0.001 / 0.001
  LaProp v 0.60 / 0.02 / 0.02    m 0.43 / 0.01 / 0.01    parameter step 0.22 / 0.04 / 0.03
  _cal_grad gradients (elements and norms) 0.06 / 0.11 / 0.06
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

from golden_io import HERE, batch, initial, sample_idx
from oracle.init import params_for
from oracle.ref_cpu import Spec
from parity import assert_close, bound_ratio, ulp
from sdreamer.config import load_config
from test_gpu_dreamer import WM_KEYS, _Sp, _Spaces, _rel

pytestmark = pytest.mark.gpu
DEV = "cuda"
OBS = {"image": (64, 64, 3)}
CASES = {"walker_mm_r2": [], "walker_mm_filmonly": ["model.multimodal_encoder.use_text_gate=False"],
         "walker_mm_gateonly": ["model.ablation_encoder_type=gate_only"]}
FRONT = "encoder.text_context_encoder."
MIN_GAP = 2e-4


def _config(name, device):
    z = dict(np.load(os.path.join(HERE, name + ".npz")))
    cfg = load_config("dmc/cnn", [f"device={device}", "model.compile=False", f"model.imag_horizon={int(z['meta_H'])}",
                                  "model.use_multimodal_encoder=True"] + CASES[name])
    return z, cfg


def _build(name):
    """the product Dreamer of a fixture with its weights by name (through load_state_dict) and its two texts"""
    from sdreamer.dreamer import Dreamer
    z, cfg = _config(name, "cuda:0")
    spec = Spec(cfg.model, OBS, int(z["meta_A"]), False)  # dims and slow-critic names; the shapes are the fixture's
    shapes = {k: tuple(v) for k, v in json.loads(str(z["meta_shapes"])).items()}
    params = params_for(shapes, int(z["meta_param_seed"]))
    ag = Dreamer(copy.deepcopy(cfg.model), _Spaces({k: _Sp(v) for k, v in OBS.items()}), _Sp((int(z["meta_A"]),)))
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    for k, sk in spec.slow_names.items():
        sd[sk] = torch.from_numpy(params[k])
    sd["return_ema.ema_vals"] = torch.zeros(2)
    missing, unexpected = ag.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert not [m for m in missing if not m.startswith("_frozen")], missing
    ag.set_text_features([str(t) for t in z["texts"]], [z["feat_0"], z["feat_1"]])
    ag.set_task_name("walker_walk")
    return ag, z, spec, shapes, params


def _force_text(ag, B, idx):
    """this update reads text `idx`: the schedule's current text, mid-interval (no new draw)"""
    enc = ag.encoder
    if enc._ctx is None:
        enc.text_context(B, ag.device, force_index=idx)
    enc._text_index, enc._forward_count = int(idx), 1


def _opt_samples(ag, shapes):
    sd = ag._optimizer.state_dict()["state"]
    ref_index = getattr(ag._optimizer, "ref_index", None)
    sd_name = {id(p): n for n, p in ag.named_parameters()}
    out = {}
    for i, prm in enumerate(ag._named_params.values()):
        k, j = sd_name[id(prm)], (ref_index[i] if ref_index is not None else i)
        if k in shapes and j in sd:
            m = sd[j]["exp_avg"].reshape(-1).cpu().numpy()
            v = sd[j]["exp_avg_sq"].reshape(-1).cpu().numpy()
            idx = sample_idx(k, m.size)
            out[k] = (m[idx], v[idx])
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_update_matches_reference(name):
    ag, z, spec, shapes, params0 = _build(name)
    assert float(z["meta_min_gap"]) >= MIN_GAP, "the fixture's seed search found no tie-free batch"
    gate = "u0_gate_mean" in z
    SK, S, Kd = spec.SK, spec.S, spec.K
    B = int(z["meta_B"])
    trainable = [k for k in shapes if not k.startswith(FRONT)]
    prev = {k: params0[k].reshape(-1)[sample_idx(k, params0[k].size)] for k in trainable}
    worst = {}

    def close(got, ref, rtol, atol, what, cls, mask=None):
        r = bound_ratio(got, ref, rtol, atol, mask=mask)
        if r > worst.get(cls, ("", 0.0))[1]:
            worst[cls] = (what, r)
        print(f"{name} {what}: {r:.4g} of the bound", flush=True)
        assert_close(got, ref, rtol, atol, what, mask=mask)

    for u in range(2):
        seed = int(z[f"u{u}_seed"])
        data = batch(z, u, OBS, DEV)
        data["image"] = torch.from_numpy(z[f"u{u}_in_image"]).to(DEV)  # uint8: exercise preprocess
        _force_text(ag, B, int(z[f"u{u}_text"]))
        (ps, pd), mets = ag.update_batch(data, initial(z, u, spec, DEV), seed)
        torch.cuda.synchronize()
        assert ag.encoder._cached_index == int(z[f"u{u}_text"])
        close(ag.encoder._ctx.cpu().numpy(), z[f"u{u}_ctx"], 1e-4, 1e-5, f"u{u} text context", "embed")
        # posterior and imagined indices: exact, no exclusions
        assert np.array_equal(ps.argmax(-1).cpu().numpy(), z[f"u{u}_post_idx"]), f"u{u} posterior indices"
        close(pd.detach().cpu().numpy()[..., ::4], z[f"u{u}_post_deter"], 1e-4, 1e-5, f"u{u} post_deter", "post_deter")
        ref_logit = z[f"u{u}_post_logit"]
        close(ag._last["post_logit"].detach().cpu().numpy(), ref_logit, 1e-4, 1e-4, f"u{u} post_logit", "logit")
        close(ag._last["prior_logit"].detach().cpu().numpy().reshape(ref_logit.shape), z[f"u{u}_prior_logit"],
              1e-4, 1e-4, f"u{u} prior_logit", "logit")
        close(ag._last["embed"].detach().cpu().numpy()[..., ::8], z[f"u{u}_embed"], 1e-4, 1e-5,
              f"u{u} visual_embed", "embed")
        close(ag._last["rssm_embed"].detach().cpu().numpy()[..., ::8], z[f"u{u}_rssm_embed"], 1e-4, 1e-5,
              f"u{u} rssm_embed", "embed")
        ifeat = ag._last["imag_feat_tm"].detach().transpose(0, 1).cpu().numpy()
        N, H1 = ifeat.shape[:2]
        assert np.array_equal(ifeat[..., :SK].reshape(N, H1, S, Kd).argmax(-1), z[f"u{u}_imag_idx"]), \
            f"u{u} imagined indices"
        close(ifeat[..., SK::16], z[f"u{u}_imag_deter"], 1e-4, 1e-5, f"u{u} imag_deter", "imagination")
        close(ag._last["imag_action_tm"].detach().transpose(0, 1).cpu().numpy(), z[f"u{u}_imag_action"], 1e-4, 1e-5,
              f"u{u} imag_action", "imagination")
        close(ag._last["ret"].detach().cpu().numpy()[..., None], z[f"u{u}_imag_ret"], 1e-3, 1e-4, f"u{u} imag_ret",
              "returns")
        close(ag._last["rret"].detach().cpu().numpy()[..., None], z[f"u{u}_replay_ret"], 1e-3, 1e-4,
              f"u{u} replay_ret", "returns")
        close(ag.return_ema.ema_vals.cpu().numpy(), z[f"u{u}_ema_vals"], 1e-4, 1e-6, f"u{u} ema_vals", "returns")
        # losses and metrics, test_update_matches_reference's classes
        bad = []
        for k, v in mets.items():
            key = f"u{u}_m_{k}"
            if key not in z:
                continue
            tol, cls = (1e-4, "wm_loss") if (k.startswith("loss/") and k[5:] in WM_KEYS) else (1e-3, "metric")
            if k.startswith("action_") or k.startswith("ret") or k in ("adv", "adv_std", "tar", "val", "rew", "slowval",
                                                                         "opt/loss") or \
                    k.startswith("value_replay") or k.startswith("slow_value_replay"):
                tol, cls = 5e-3, "metric_5e-3"
            r = _rel(v, z[key])
            if abs(float(v) - float(z[key])) > 1e-5 and r / tol > worst.get(cls, ("", 0.0))[1]:
                worst[cls] = (f"u{u} {k}", r / tol)
            if r > tol and abs(float(v) - float(z[key])) > 1e-5:
                bad.append((k, float(v), float(z[key]), r))
        assert not bad, bad
        if gate:  # the gate's mean / unbiased std were among the metrics compared above
            for k in ("encoder/text_gate_mean", "encoder/text_gate_std", "encoder/text_gate_final_bias_mean",
                      "encoder/text_gate_final_weight_norm", "encoder/text_proj_weight_norm"):
                assert f"u{u}_m_{k}" in z and k in mets, k
        # LaProp moments and the parameter step of every trainable tensor (bounds: test_update_matches_reference)
        opt = _opt_samples(ag, shapes)
        assert not [k for k in opt if k.startswith(FRONT)]  # no state for the text front end
        sd = ag.state_dict()
        for k in trainable:
            assert k in opt, f"no optimizer state for {k}"
            m, v = opt[k]
            m_ref, v_ref = z[f"u{u}_st_{k}__m"], z[f"u{u}_st_{k}__v"]
            tiny = np.sqrt(v_ref) < 1e-3 * np.sqrt(v_ref).max()
            close(v, v_ref, 2e-2, 2e-4 * np.abs(v_ref).max() + 1e-30, f"u{u} exp_avg_sq {k}", "v")
            close(m, m_ref, 2e-2, 1e-2 * np.abs(m_ref).max() + 1e-30, f"u{u} exp_avg {k}", "m", mask=tiny)
            flat = sd[k].detach().reshape(-1).cpu().numpy()
            ref = z[f"u{u}_p_{k}__s"]
            d_got = flat[sample_idx(k, flat.size)].astype(np.float64) - prev[k]
            d_ref = ref.astype(np.float64) - prev[k]
            close(d_got, d_ref, 2e-2, 1e-2 * np.abs(d_ref).max() + 4 * ulp(ref), f"u{u} parameter step {k}", "step",
                  mask=tiny)
            prev[k] = ref.astype(np.float64)
        for k in shapes:  # the four text front-end tensors: unchanged to the bit
            if k.startswith(FRONT):
                assert f"u{u}_nostate__{k}" in z
                assert np.array_equal(sd[k].cpu().numpy(), params0[k]), k
        for k, sk in spec.slow_names.items():
            flat = sd[sk].detach().reshape(-1).cpu().numpy()
            ref = z[f"u{u}_p_{sk}__s"]
            assert_close(flat[sample_idx(sk, flat.size)], ref, 0.0, 4 * ulp(ref) + 1e-12, f"u{u} slow critic {sk}")
    print(name, "worst bound ratio per class:", json.dumps({c: {"what": w, "ratio": round(r, 4)}
                                                             for c, (w, r) in sorted(worst.items())}))


@pytest.mark.parametrize("name", list(CASES))
def test_cal_grad_matches_reference(name):
    """Gradients of one _cal_grad at the initial weights with a text context whose two rows differ (row b: the context
    of text b), vs the reference's: elements within 2e-3 relative + 1e-4 of the tensor's largest sampled |g|, norms
    within 2e-4."""
    ag, z, spec, shapes, _ = _build(name)
    ag.use_graphs = False
    ctx = torch.from_numpy(z["g_text_ctx"]).to(DEV)
    assert not torch.equal(ctx[0], ctx[1])
    with torch.no_grad():  # the product's own front end gives the same two rows
        rows = torch.cat([ag.encoder.text_context_encoder(torch.from_numpy(z[f"feat_{i}"]).to(DEV)) for i in (0, 1)])
    assert_close(rows.cpu().numpy(), z["g_text_ctx"], 1e-4, 1e-5, "per-row text context")
    data = ag.preprocess(batch(z, 0, OBS, DEV))
    ag._update_slow_target()
    ag._optimizer.zero_grad()
    ag._text_ctx = ctx.contiguous()
    ag._cal_grad(data, initial(z, 0, spec, DEV), 1000, 0)
    torch.cuda.synchronize()
    named = dict(ag.named_parameters())
    bad, worst = [], (0.0, None)
    for k in shapes:
        g = named[k].grad
        if k.startswith(FRONT):
            assert f"g_none__{k}" in z and (g is None or not g.any()), k
            continue
        assert g is not None, k
        flat = ag.to_ref_layout(named[k], g).reshape(-1).double().cpu().numpy()
        ref_n, ref = float(z[f"g_{k}__n"]), z[f"g_{k}__s"].astype(np.float64)
        n = float(np.linalg.norm(flat))
        if abs(n - ref_n) > 2e-4 * max(ref_n, 1e-9) and abs(n - ref_n) > 1e-9:
            bad.append((k, "norm", n, ref_n))
        got = flat[sample_idx(k, flat.size)]
        scale = np.abs(ref).max()
        err = np.abs(got - ref) - (2e-3 * np.abs(ref) + 1e-4 * scale + 1e-12)
        if err.max() > 0:
            i = int(np.argmax(err))
            bad.append((k, "element", float(got[i]), float(ref[i])))
        r = bound_ratio(got, ref, 2e-3, 1e-4 * scale + 1e-12)
        rn = abs(n - ref_n) / (2e-4 * max(ref_n, 1e-9))
        if max(r, rn) > worst[0]:
            worst = (max(r, rn), k)
    print(name, "worst fraction of a gradient bound used", worst)
    assert not bad, bad


@pytest.mark.parametrize("name", list(CASES))
def test_weight_init_matches_reference(name):
    """Dreamer's own initialisation vs the reference's initialisers run under torch.manual_seed(0) (fixture
    init_*__stat: mean, std, max|w|, numel per tensor), for every tensor the multimodal switch adds or replaces
    (encoder.*, prj.*). The draws differ, so the test is distributional: constants (zero biases, zero last FiLM / gate
    layers, the gate's bias, unit norm scales) exact; std within 4/sqrt(n) + 1 %, mean within 6 std/sqrt(n); max|w|
    no larger than the reference's bound — the uniform's half-width a = std sqrt(3) for the Xavier-uniform layers
    (max|w| >= 0.9 a tells them from a truncated normal), 2 sigma for the truncated-normal conv layers — and at least
    half the reference's."""
    from sdreamer.dreamer import Dreamer
    z, cfg = _config(name, "cuda:0")
    shapes = {k: tuple(v) for k, v in json.loads(str(z["meta_shapes"])).items()}
    torch.manual_seed(0)
    ag = Dreamer(copy.deepcopy(cfg.model), _Spaces({k: _Sp(v) for k, v in OBS.items()}), _Sp((int(z["meta_A"]),)))
    sd = ag.state_dict()
    keys = [k for k in shapes if k.startswith(("encoder.", "prj."))]
    assert len(keys) >= 13
    bad = []
    for k in keys:
        mean_r, std_r, amax_r, n = (float(x) for x in z[f"init_{k}__stat"])
        w = sd[k].detach().double().reshape(-1).cpu()
        assert w.numel() == int(n), k
        mean, std, amax = w.mean().item(), (w.std().item() if w.numel() > 1 else 0.0), w.abs().max().item()
        if std_r == 0.0:
            if not (mean == mean_r and amax == amax_r):
                bad.append((k, "constant", mean, mean_r))
            continue
        if abs(std / std_r - 1) > 4 / np.sqrt(n) + 0.01:
            bad.append((k, "std", std, std_r))
        if abs(mean - mean_r) > 6 * std_r / np.sqrt(n):
            bad.append((k, "mean", mean, mean_r))
        uniform = amax_r < 1.8 * std_r  # U(-a, a): max = 1.732 std; a normal truncated at 2 sigma: 2.27 std
        limit = std_r * 3 ** 0.5 if uniform else 2 * std_r / 0.8796
        if amax > max(limit * (1 + 4 / np.sqrt(n)), amax_r) * 1.001 or amax < 0.5 * amax_r:
            bad.append((k, "max", amax, amax_r))
        if uniform and amax < 0.9 * amax_r:
            bad.append((k, "uniform", amax, amax_r))
    assert not bad, bad
