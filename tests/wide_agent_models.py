"""The wide-encoder agent case: dmc/cnn with model.depth=33 (stages 66 / 99 / 132 / 132: two stages above 128
channels, an odd input width, one that is no multiple of 4) at B2 x T4 x H3, against oracle/ref_cpu.OracleAgent in
float64 (ref_cpu.DT, switched by small_models.oracle_dtype). Test infrastructure (a plain module), shared by
tests/test_wide_agent_cpu.py (the seed's input condition) and tests/test_gpu_wide_agent.py (the product).

Everything is regenerated from the seed: parameters (oracle/init.py params_for), the two updates' batches and initial
latents, the Philox noise seeds. Index rule: EXACT equality. The seed is the first whose smallest top-two
perturbed-logit margin (posterior and imagined samples of both updates) under the float32 oracle is >= MIN_MARGIN and
whose float32 and float64 oracles draw the same indices; the CPU file enforces it.
"""
import functools

import numpy as np
import torch

import small_models as sm
from oracle import ref_cpu
from oracle.init import params_for
from parity import imag_margins, post_margins
from sdreamer.config import load_config

CONFIG, DEPTH = "dmc/cnn", 33
B, T, H, A = 2, 4, 3, 6
OBS = {"image": (64, 64, 3)}
OVERRIDES = [f"model.depth={DEPTH}", f"model.imag_horizon={H}", "model.compile=False"]
MIN_MARGIN = sm.MIN_MARGIN  # 1e-4
MAX_SEEDS = 16
SEED = 0  # the first seed that meets the input condition (test_wide_agent_cpu.py)
UPDATES = 2
WM_KEYS = ("dyn", "rep", "barlow", "rew", "con")


@functools.lru_cache(maxsize=None)
def spec_params(seed):
    cfg = load_config(CONFIG, ["device=cpu"] + OVERRIDES)
    spec = ref_cpu.Spec(cfg.model, OBS, A, False)
    assert tuple(DEPTH * m for m in (2, 3, 4, 4)) == (66, 99, 132, 132)
    return spec, params_for(spec.shapes, seed)


def noise_seed(seed, u):
    return 1000 + 77 * seed + u


@functools.lru_cache(maxsize=None)
def inputs(seed, u):
    """update u's replay batch (uint8 images, actions, rewards, episode flags) and initial latents, numpy"""
    spec, _ = spec_params(seed)
    rng = np.random.default_rng([seed, u, 33])
    d = {"image": rng.integers(0, 256, size=(B, T, 64, 64, 3), dtype=np.uint8),
         "action": rng.uniform(-1, 1, size=(B, T, A)).astype(np.float32),
         "reward": rng.uniform(0, 1, size=(B, T, 1)).astype(np.float32)}
    first = np.zeros((B, T, 1), bool)
    first[:, 0] = True
    first[1, 2] = True  # a reset inside the sequence
    d["is_first"] = first
    term = np.zeros((B, T, 1), bool)
    term[0, T - 1] = True
    d["is_terminal"], d["is_last"] = term, term.copy()
    idx = rng.integers(0, spec.K, size=(B, spec.S))
    init = (np.eye(spec.K, dtype=np.float32)[idx], (0.5 * rng.standard_normal((B, spec.D))).astype(np.float32))
    return d, init


def _oracle_batch(seed, u, dtype):
    d, init = inputs(seed, u)
    data = {k: torch.from_numpy(v) for k, v in d.items()}
    data["image"] = (data["image"].float() / 255.0).to(dtype)  # the f32 value the reference forms, then the cast
    for k in ("action", "reward"):
        data[k] = data[k].to(dtype)
    return data, tuple(torch.from_numpy(v).to(dtype) for v in init)


@functools.lru_cache(maxsize=None)
def run_oracle(seed, dtype=torch.float64):
    """UPDATES OracleAgent.update()s: per update the posterior / imagined indices, the smallest perturbed-logit margin
    and the losses"""
    spec, params = spec_params(seed)
    out = []
    with sm.oracle_dtype(dtype):
        orc = ref_cpu.OracleAgent(spec, params)
        for u in range(UPDATES):
            data, init = _oracle_batch(seed, u, dtype)
            keep = {}
            (ps, _), losses, _ = orc.update(data, init, noise_seed(seed, u), keep=keep)
            feat = keep["imag_feat"].detach().numpy()  # (N, H + 1, F)
            N, H1 = feat.shape[:2]
            pm = post_margins(keep["post_logit"].detach().numpy(), noise_seed(seed, u), spec.unimix)
            im = imag_margins(keep["imag_prior_logit"].detach().numpy(), noise_seed(seed, u), spec.unimix)
            out.append(dict(post_idx=ps.detach().argmax(-1).numpy(),
                            imag_idx=feat[..., :spec.SK].reshape(N, H1, spec.S, spec.K).argmax(-1),
                            margin=float(min(pm.min(), im.min())),
                            losses={k: float(v.detach()) for k, v in losses.items()}))
    return out


@functools.lru_cache(maxsize=None)
def oracle_encoder_grads(seed, dtype=torch.float64):
    """the encoder's parameter gradients (reference names / layouts) of one cal_grad at the initial weights"""
    spec, params = spec_params(seed)
    with sm.oracle_dtype(dtype):
        orc = ref_cpu.OracleAgent(spec, params)
        orc.update_slow_target()
        data, init = _oracle_batch(seed, 0, dtype)
        orc.cal_grad(data, init, noise_seed(seed, 0))
        return {k: orc.P[k].grad.detach().double().numpy() for k in spec.shapes if k.startswith("encoder.")}


def meets_condition(seed):
    r32, r64 = run_oracle(seed, torch.float32), run_oracle(seed, torch.float64)
    same = all(np.array_equal(a[k], b[k]) for a, b in zip(r32, r64) for k in ("post_idx", "imag_idx"))
    return min(r["margin"] for r in r32) >= MIN_MARGIN and same


class Sp:
    def __init__(self, shape):
        self.shape = tuple(shape)


class Spaces:
    def __init__(self, d):
        self.spaces = d


def build_product(seed, depth=DEPTH, extra=()):
    """The product Dreamer with the seed's parameters loaded through load_state_dict (the checkpoint layout)"""
    import copy

    from sdreamer.dreamer import Dreamer
    ovr = [o for o in OVERRIDES if not o.startswith("model.depth=")] + [f"model.depth={depth}"] + list(extra)
    gcfg = load_config(CONFIG, ["device=cuda:0"] + ovr)
    ag = Dreamer(copy.deepcopy(gcfg.model), Spaces({k: Sp(v) for k, v in OBS.items()}), Sp((A,)))
    if depth == DEPTH:
        spec, params = spec_params(seed)
        sd = {k: torch.from_numpy(v) for k, v in params.items()}
        for k, sk in spec.slow_names.items():
            sd[sk] = torch.from_numpy(params[k])
        sd["return_ema.ema_vals"] = torch.zeros(2)
        missing, unexpected = ag.load_state_dict(sd, strict=False)
        assert not unexpected, unexpected
        assert not [m for m in missing if not m.startswith("_frozen")], missing
    return ag


def product_batch(seed, u, dev="cuda"):
    d, init = inputs(seed, u)
    return {k: torch.from_numpy(v).to(dev) for k, v in d.items()}, tuple(torch.from_numpy(v).to(dev) for v in init)
