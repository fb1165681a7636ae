"""The image-gradient probe on the CPU oracle (oracle/ref_cpu.py: encode + observe under autograd), shared by the
fixture generator, the CPU fixture test and the GPU tests: loss = mean(dyn) + mean(rep) + <post_deter, R> with
dyn, rep the two KL terms without free bits, differentiated back to the float image."""
import os
import zlib

import numpy as np
import torch

from golden_io import HERE, sample_idx
from oracle import ref_cpu

N_SAMPLE = 4096


def load_fixture(name="walker_r2_imgrad"):
    return np.load(os.path.join(HERE, name + ".npz"), allow_pickle=False)


def probe_R(B, T, D):
    return np.random.default_rng(zlib.crc32(b"imgrad")).standard_normal((B, T, D)).astype(np.float32)


def fixture_inputs(z, obs, spec, device="cpu"):
    """(data, initial) of the fixture's batch: image float in [0, 1] as Dreamer.preprocess forms it"""
    data = {}
    for k in list(obs) + ["action", "reward", "is_first", "is_terminal", "is_last"]:
        v = torch.from_numpy(z[f"in_{k}"])
        data[k] = (v.float() / 255.0 if k in obs and len(obs[k]) == 3 else v).to(device)
    stoch = torch.nn.functional.one_hot(torch.from_numpy(z["in_init_stoch"].astype(np.int64)), spec.K).float()
    return data, (stoch.to(device), torch.from_numpy(z["in_init_deter"]).to(device))


def sampled(g):
    """(per-frame L2 norms (B, T), the N_SAMPLE sampled elements) of an image gradient (B, T, H, W, C), float64"""
    g = np.asarray(g, dtype=np.float64)
    return np.sqrt((g ** 2).sum((2, 3, 4))), g.reshape(-1)[sample_idx("imgrad", g.size, N_SAMPLE)]


def probe_loss_terms(dyn, rep, post_deter, R):
    return dyn.mean() + rep.mean() + (post_deter * R).sum()


def oracle_image_grad(spec, params, data, init, seed, R, dt=torch.float32):
    """-> (d loss / d image as a float64 array, posterior indices, loss) of the oracle in dtype dt (inputs are the f32
    values the product sees, cast)"""
    ref_cpu.DT = dt
    try:
        ag = ref_cpu.OracleAgent(spec, params)
        M = ag.model
        cast = lambda t: t.to(dt) if t.is_floating_point() else t  # noqa: E731
        d = {k: cast(v) for k, v in data.items()}
        d["image"] = d["image"].clone().requires_grad_()
        ini = tuple(cast(t) for t in init)
        embed = M.encode(d)
        post_stoch, post_deter, post_logit = M.observe(embed, d["action"], ini, d["is_first"], seed)
        prior_logit = M.img_logit(post_deter)
        rep = ref_cpu.kl_cat(post_logit, prior_logit.detach()).sum(-1)
        dyn = ref_cpu.kl_cat(post_logit.detach(), prior_logit).sum(-1)
        loss = probe_loss_terms(dyn, rep, post_deter, torch.as_tensor(R).to(dt))
        loss.backward()
        return (d["image"].grad.double().numpy(), post_stoch.detach().argmax(-1).numpy().astype(np.int16),
                float(loss.detach()))
    finally:
        ref_cpu.DT = torch.float32


def distance(norms, elems, ref_norms, ref_elems):
    """(worst per-frame norm error relative to the reference norm, worst element error in units of the gradient
    test's bound 2e-3 |ref| + 1e-4 max |ref|)"""
    dn = float((np.abs(norms - ref_norms) / np.maximum(ref_norms, 1e-30)).max())
    bound = 2e-3 * np.abs(ref_elems) + 1e-4 * np.abs(ref_elems).max()
    return dn, float((np.abs(elems - ref_elems) / bound).max())
