"""observation_grad at B16 L64 (Nb = 1024) and the first stage's input gradient alone: sd_conv2d_dgrad_pool vs the
fallback's two launches on the same inputs (device events, alternating rounds). GPU box, repo root:
    python tools/imgrad_bench.py        (under rocprofv3 --kernel-trace --stats for the per-kernel table)"""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "safe-dreamer_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from sdreamer import kernels as K  # noqa: E402
from sdreamer.config import load_config  # noqa: E402
from sdreamer.dreamer import Dreamer  # noqa: E402


class Sp:
    def __init__(self, s):
        self.shape = tuple(s)


class Spaces:
    def __init__(self, d):
        self.spaces = d


def ev_time(fn, reps):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps * 1e3


def main():
    torch.manual_seed(0)
    dev = "cuda:0"
    B, T = 16, 64
    cfg = load_config("dmc/cnn", ["device=cuda:0", "model.compile=False"])
    ag = Dreamer(copy.deepcopy(cfg.model), Spaces({"image": Sp((64, 64, 3))}), Sp((6,)))
    g = torch.Generator().manual_seed(1)
    data = {"image": torch.randint(0, 256, (B, T, 64, 64, 3), generator=g, dtype=torch.uint8).to(dev),
            "action": (torch.rand(B, T, 6, generator=g) * 2 - 1).to(dev),
            "is_first": torch.zeros(B, T, 1, dtype=torch.bool).to(dev)}
    data["is_first"][:, 0] = True
    init = ag.rssm.initial(B)
    R = torch.randn(B, T, ag.rssm._deter, generator=g).to(dev)

    def loss_fn(ps, pd, pl):
        dyn, rep = ag.rssm.kl_loss(pl, ag.rssm.prior(pd), 0.0)
        return dyn.mean() + rep.mean() + (pd * R).sum()

    takes = K.conv2d_dgrad_pool_takes
    res = {}
    for name, fn in (("kernel", takes), ("fallback", lambda *a, **k: False)):
        K.conv2d_dgrad_pool_takes = fn
        for _ in range(3):
            ag.observation_grad(data, init, loss_fn, seed=3)
        torch.cuda.synchronize()
        res[name] = ev_time(lambda: ag.observation_grad(data, init, loss_fn, seed=3), 10)
    K.conv2d_dgrad_pool_takes = takes
    print(f"observation_grad B{B} L{T}: first-stage dx by the pooled-gradient kernel {res['kernel']:.0f} us, "
          f"by the fallback {res['fallback']:.0f} us per call", flush=True)

    # the first stage alone, same inputs
    Nb = B * T
    x = K.pad_channels(torch.rand(Nb, 64, 64, 3, generator=g).to(dev), 4, 0.5)
    w = (torch.randn(32, 5, 5, 3, generator=g) / 75 ** 0.5).to(dev)
    wp = torch.zeros(32, 5, 5, 4, device=dev)
    wp[..., :3] = w
    b, nw = torch.zeros(32, device=dev), torch.ones(32, device=dev)
    y, pooled, amax, rstd = K.conv2d_fwd_pool(x, wp, b, nw)
    dy = torch.randn(y.shape, generator=g).to(dev)
    dnw = torch.zeros(32, device=dev)
    dpool = K.pool_rms_bwd_compact(pooled, amax, nw, rstd, dy, dnw)
    keep = K.set_flip_cache([wp])

    def new():
        return K.conv2d_dgrad_pool(dpool, amax, w)

    def old_a():
        return K.pool_rms_bwd(pooled, amax, nw, rstd, dy, 64, 64, dnw)

    dconv = old_a()

    def old_b():
        return K.conv2d_dgrad(dconv, wp)

    a, r = new(), old_b()[..., :3]
    torch.cuda.synchronize()
    print("new vs fallback dx: max |diff|", float((a - r).abs().max()), "max |dx|", float(r.abs().max()), flush=True)
    for _ in range(3):
        new(), old_a(), old_b()
    torch.cuda.synchronize()
    rows = []
    for rep in range(5):  # alternating
        rows.append((ev_time(new, 20), ev_time(old_a, 20), ev_time(old_b, 20)))
    for t in rows:
        print(f"first stage dx at Nb={Nb}: sd_conv2d_dgrad_pool {t[0]:.1f} us | sd_pool_rms_bwd {t[1]:.1f} us + padded "
              f"conv2d_dgrad {t[2]:.1f} us = {t[1] + t[2]:.1f} us", flush=True)
    del keep


if __name__ == "__main__":
    main()
