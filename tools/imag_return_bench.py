"""Dreamer.imagined_return forward + backward at B16 L64 H15 (N = 1,024 start rows): device-event times of the whole,
the forward, the backward's phases (returns + heads, batched recompute, the serial walk) and the ABI calls per serial
step; beside them the imagination forward alone and observation_grad. GPU box, repo root:
    python tools/imag_return_bench.py        (under rocprofv3 --kernel-trace --stats for the per-kernel table)"""
import collections
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "safe-dreamer_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from sdreamer import _native as nat  # noqa: E402
from sdreamer import ops  # noqa: E402
from sdreamer.config import load_config  # noqa: E402
from sdreamer.dreamer import Dreamer  # noqa: E402


class Sp:
    def __init__(self, s):
        self.shape = tuple(s)


class Spaces:
    def __init__(self, d):
        self.spaces = d


class Launches:
    """counts C-ABI launches by name while in nat.PROBES (matches none, so times none)"""

    def __init__(self):
        self.names = []

    def match(self, name, args):
        self.names.append(name)
        return False


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
    r = ag.rssm
    N, H1 = B * T, ag.imag_horizon + 1
    g = torch.Generator().manual_seed(1)
    idx = torch.randint(0, r._discrete, (N, r._stoch), generator=g)
    stoch = torch.nn.functional.one_hot(idx, r._discrete).float().to(dev)
    deter = (0.5 * torch.randn(N, r._deter, generator=g)).to(dev)

    def fwd_bwd():
        s, d = stoch.clone().requires_grad_(True), deter.clone().requires_grad_(True)
        ag.imagined_return(s, d, seed=3).mean().backward()
        return s.grad, d.grad

    def fwd():
        with torch.no_grad():
            return ag.imagined_return(stoch, deter, seed=3)

    def imag():
        with torch.no_grad():
            return ag._imagine_tm((stoch.reshape(N, -1), deter), H1, 3)

    for _ in range(3):
        fwd_bwd()
    torch.cuda.synchronize()
    print(f"N {N} H1 {H1} D {r._deter} SK {r.flat_stoch} fused imagination {bool(ag._fused_imag_ok())}", flush=True)
    for rep in range(3):
        print(f"imagined_return forward + backward {ev_time(fwd_bwd, 5):.0f} us | forward {ev_time(fwd, 5):.0f} us | "
              f"imagination forward alone {ev_time(imag, 5):.0f} us", flush=True)

    # the backward's phases
    ops.IMAG_RETURN_MARKS = marks = []
    fwd_bwd()
    torch.cuda.synchronize()
    ops.IMAG_RETURN_MARKS = None
    t = [(a, m[1].elapsed_time(n[1]) * 1e3) for a, m, n in zip([n[0] for n in marks[1:]], marks[:-1], marks[1:])]
    steps = [v for a, v in t if a == "step"]  # the per-op walk marks every step, the fused walk its one ABI call
    walk = [v for a, v in t if a == "walk"]
    total = sum(v for _, v in t)
    H = ag.imag_horizon
    serial = (f"{len(steps)} serial steps {sum(steps):.0f} us (mean {sum(steps) / len(steps):.0f} us, min "
              f"{min(steps):.0f}, max {max(steps):.0f})" if steps else
              f"fused serial walk of {H} steps {sum(walk):.0f} us (mean {sum(walk) / H:.0f} us a step)")
    print(f"backward {total:.0f} us: returns + heads {t[0][1]:.0f} us, batched recompute {t[1][1]:.0f} us "
          f"({100 * t[1][1] / total:.1f} %), {serial}", flush=True)

    # launches: the whole backward, and one serial step (the difference between horizons H and H - 1)
    def launches(h):
        s, d = stoch.clone().requires_grad_(True), deter.clone().requires_grad_(True)
        ret = ag.imagined_return(s, d, horizon=h, seed=3).mean()
        rec = Launches()
        nat.PROBES.append(rec)
        try:
            ret.backward()
            torch.cuda.synchronize()
        finally:
            nat.PROBES.remove(rec)
        return collections.Counter(rec.names)

    a, b = launches(ag.imag_horizon), launches(ag.imag_horizon - 1)
    per_step = a - b
    print(f"ABI calls in the backward at H {ag.imag_horizon}: {sum(a.values())}; per serial step "
          f"{sum(per_step.values())}: {dict(per_step)} (sd_imagine_bwd: {a['sd_imagine_bwd']} call(s) for all steps; its "
          f"kernels per step are in the kernel trace)", flush=True)


if __name__ == "__main__":
    main()
