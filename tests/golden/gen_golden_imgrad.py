"""Golden vector of the reference's gradient with respect to its image input (tests/golden/walker_r2_imgrad.npz).

Runs where the reference is importable only (see refimport.py); the fixture it writes is data. The reference `Dreamer`
of the walker_r2 case (gen_golden.py: dmc/cnn, B2 T6, weights by name, injected Gumbel noise of seed 1000) runs its own
encoder and `rssm.observe` on a float image that requires grad, then the probe loss

    mean(dyn) + mean(rep) + <post_deter, R>,   dyn, rep = rssm.kl_loss(post_logit, prior_logit, free=0)

with prior_logit = rssm.prior(post_deter)[1] and R ~ N(0, 1) from default_rng(crc32("imgrad")), and `.backward()` to
the image. Stored: the gradient's L2 norm per frame, 4,096 sampled elements (golden_io.sample_idx's scheme), the
posterior indices, R, and the same gradient from the CPU oracle (oracle/ref_cpu.py) in float64 on the same f32 inputs
(the reference casts its logits to f32, so it has no float64 run of its own). The batch seed is
crc32("walker_r2") + k for the first k in 0..50 whose smallest top-two gap of `logits + g` over the posterior draws is
>= 2e-4 (k = 0 is the walker_r2 case's own update-0 batch); k, the gap and the inputs are stored.

    python tests/golden/gen_golden_imgrad.py
"""
import contextlib
import copy
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "safe-dreamer_amd"), os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

from imgrad_ref import fixture_inputs, oracle_image_grad, probe_R, sampled  # noqa: E402
from oracle.init import params_for  # noqa: E402
from refimport import import_reference  # noqa: E402

NAME, CASE = "walker_r2_imgrad", "walker_r2"
MIN_GAP, MAX_K, SEED = 2e-4, 50, 1000


class _Sp:
    def __init__(s, shape):
        s.shape = shape


class _Spaces:
    def __init__(s, d):
        s.spaces = d


def build(mods):
    from gen_golden import CASES, PARAM_SEED
    from oracle.ref_cpu import Spec
    from sdreamer.config import load_config
    cfg_name, ovr, obs, A, discrete, B, T, H = CASES[CASE]
    cfg = load_config(cfg_name, ["device=cpu", "model.compile=False", f"model.imag_horizon={H}"] + ovr)
    ag = mods["world_model.dreamer"].Dreamer(copy.deepcopy(cfg.model), _Spaces({k: _Sp(v) for k, v in obs.items()}),
                                             _Sp((A,)))
    spec = Spec(cfg.model, obs, A, discrete)
    vals = params_for(spec.shapes, PARAM_SEED)
    named = dict(ag.named_parameters())
    with torch.no_grad():
        for k, v in vals.items():
            named[k].data.copy_(torch.from_numpy(v))
    return ag, spec, vals, (obs, A, discrete, B, T, H)


@contextlib.contextmanager
def noise(seq, gaps):
    """gen_golden.py's stand-in for F.gumbel_softmax; `gaps` collects the top-two gap of logits + g of the posterior
    draws (the prior's draw is discarded by the reference)"""
    orig = torch.nn.functional.gumbel_softmax

    def gs(logits, tau=1, hard=False, eps=1e-10, dim=-1):
        used = seq.g != seq.T
        g = torch.from_numpy(seq.gumbel(tuple(logits.shape)))
        if used:
            top = torch.topk(logits.detach() + g, 2, dim=dim).values
            gaps.append(float((top[..., 0] - top[..., 1]).min()))
        y_soft = ((logits + g) / tau).softmax(dim)
        index = y_soft.max(dim, keepdim=True)[1]
        y_hard = torch.zeros_like(logits).scatter_(dim, index, 1.0)
        return y_hard - y_soft.detach() + y_soft

    torch.nn.functional.gumbel_softmax = gs
    try:
        yield
    finally:
        torch.nn.functional.gumbel_softmax = orig


def run(ag, data_np, init_np, dims, R):
    """the reference's encoder -> observe -> probe loss -> backward -> (image gradient, posterior indices, loss, gap)"""
    from gen_golden import NoiseSeq
    obs, A, discrete, B, T, H = dims
    seq = NoiseSeq(T, H + 1, SEED)
    seq.discrete_act = discrete
    gaps = []
    data = ag.preprocess({k: torch.from_numpy(v) for k, v in data_np.items()})
    data["image"].requires_grad_()
    init = tuple(torch.from_numpy(v) for v in init_np)
    with noise(seq, gaps):
        embed = ag.encoder(data)
        post_stoch, post_deter, post_logit = ag.rssm.observe(embed, data["action"], init, data["is_first"])
        _, prior_logit = ag.rssm.prior(post_deter)
    dyn, rep = ag.rssm.kl_loss(post_logit, prior_logit, 0.0)
    loss = dyn.mean() + rep.mean() + (post_deter * torch.from_numpy(R)).sum()
    loss.backward()
    return (data["image"].grad.detach().numpy(), post_stoch.argmax(-1).numpy().astype(np.int16), float(loss),
            min(gaps))


def main():
    from gen_golden import make_batch, make_initial
    torch.set_num_threads(8)
    mods, _ = import_reference()
    mods["world_model.dreamer"].autocast = lambda **kw: contextlib.nullcontext()
    torch.manual_seed(0)
    ag, spec, vals, dims = build(mods)
    obs, A, discrete, B, T, H = dims
    R = probe_R(B, T, spec.D)
    best = None
    for k in range(MAX_K + 1):
        rng = np.random.default_rng(zlib.crc32(CASE.encode()) + k)
        data_np = make_batch(rng, obs, A, discrete, B, T)
        init_np = make_initial(rng, spec.S, spec.K, spec.D, B)
        res = run(ag, data_np, init_np, dims, R)
        print("k", k, "smallest top-two gap", res[3], flush=True)
        if best is None or res[3] > best[0][3]:
            best = (res, k, data_np, init_np)
        if res[3] >= MIN_GAP:
            break
    (g, idx, loss, gap), k, data_np, init_np = best
    out = {"meta_seed_k": np.int64(k), "meta_min_gap": np.float64(gap), "seed": np.int64(SEED), "R": R,
           "post_idx": idx, "loss": np.float64(loss)}
    out["g_norm"], out["g_s"] = sampled(g)
    out["g_s"] = out["g_s"].astype(np.float32)
    for kk, v in data_np.items():
        out[f"in_{kk}"] = v
    out["in_init_stoch"] = init_np[0].argmax(-1).astype(np.int16)
    out["in_init_deter"] = init_np[1]
    data, init = fixture_inputs(out, obs, spec)
    g64, idx64, loss64 = oracle_image_grad(spec, vals, data, init, SEED, R, torch.float64)
    assert np.array_equal(idx, idx64)
    out["loss64"] = np.float64(loss64)
    out["g64_norm"], out["g64_s"] = sampled(g64)
    path = os.path.join(HERE, f"{NAME}.npz")
    np.savez_compressed(path, **out)
    print(NAME, "->", path, os.path.getsize(path) // 1024, "KB; k", k, "gap", gap, "loss", loss, loss64)


if __name__ == "__main__":
    main()
