"""The resampling patch kernels in the attack loop, and what the affine / photometric EoT buys. GPU box, repo root:
    python tools/patch_affine_bench.py train on|off [steps]   a short train_patch at B16 L64 (w_return 1, 2 EoT copies:
                                                              Nb = 3,072), the eot_* ranges on or off; device-event time
                                                              of a step and of the patch entry points (run it under
                                                              rocprofv3 --kernel-trace --stats for the per-kernel table)
    python tools/patch_affine_bench.py robust                 walker_r2 weights, B2 T6: 20 steps at lr 0.05 from gray
                                                              (w_return 1, w_kl 0, w_tv 0) with the ranges off and on,
                                                              both patches under evaluate_patch(transforms=True) at a
                                                              held-out seed"""
import copy
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "safe-dreamer_amd"), os.path.join(ROOT, "tests")]

import torch  # noqa: E402

from sdreamer import kernels as K  # noqa: E402
from sdreamer.attack import EVAL_KEYS, evaluate_patch, load_attack_config, train_patch  # noqa: E402
from sdreamer.config import load_config  # noqa: E402
from sdreamer.dreamer import Dreamer  # noqa: E402

RANGES = ["eot_scale=[0.8,1.25]", "eot_rotation=20", "eot_contrast=0.2", "eot_brightness=0.1"]
PATCH_ENTRIES = ("sd_patch_apply", "sd_patch_grad", "sd_patch_apply_affine", "sd_patch_grad_affine")


class Sp:
    def __init__(self, s):
        self.shape = tuple(s)


class Spaces:
    def __init__(self, d):
        self.spaces = d


def train(ranges_on, steps):
    torch.manual_seed(0)
    dev = "cuda:0"
    B, T = 16, 64
    cfg = load_config("dmc/cnn", ["device=cuda:0", "model.compile=False"])
    ag = Dreamer(copy.deepcopy(cfg.model), Spaces({"image": Sp((64, 64, 3))}), Sp((6,)))
    g = torch.Generator().manual_seed(1)
    data = {"image": torch.randint(0, 256, (B, T, 64, 64, 3), dtype=torch.uint8, generator=g).to(dev),
            "action": (torch.rand(B, T, 6, generator=g) * 2 - 1).to(dev),
            "is_first": torch.zeros(B, T, dtype=torch.bool, device=dev)}
    data["is_first"][:, 0] = True
    init = ag.rssm.initial(B)
    over = ["w_return=1.0", "w_kl=0.0", "w_tv=0.01", "eot_translations=2"] + (RANGES if ranges_on else [])
    train_patch(ag, [(data, init)], load_attack_config(over + ["steps=2"]))  # warm-up
    torch.cuda.synchronize()
    probes = [K.LaunchProbe(n, lambda a: True, lambda a: 0.0) for n in PATCH_ENTRIES]
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    train_patch(ag, [(data, init)], load_attack_config(over + [f"steps={steps}"]))
    e.record()
    torch.cuda.synchronize()
    print(f"ranges {'on' if ranges_on else 'off'}: Nb {3 * B * T}, {steps} attack steps, {s.elapsed_time(e) / steps:.2f} ms "
          f"per step (entry-point probes attached)", flush=True)
    for pr in probes:
        pr.stop()
        ms = sorted(a.elapsed_time(b) for a, b, _ in pr.records)
        if ms:
            print(f"  {pr.name}: {len(ms)} launches, median {1e3 * ms[len(ms) // 2]:.1f} us, min {1e3 * ms[0]:.1f} us "
                  f"(device events around the entry point)", flush=True)


def robust():
    from golden_io import batch, initial
    from test_gpu_dreamer import build_agent
    dev = "cuda"
    ag, z, spec, obs = build_agent("walker_r2")
    batches = [(batch(z, 0, obs, dev), initial(z, 0, spec, dev))]
    base = ["w_return=1.0", "w_kl=0.0", "w_action=0.0", "w_tv=0.0", "steps=20", "lr=0.05", "eot_translations=2"]
    on = load_attack_config(base + RANGES)
    patches = {"gray": torch.full((16, 16, 3), 0.5, device=dev),
               "ranges off": train_patch(ag, batches, load_attack_config(base))[0].clone(),
               "ranges on": train_patch(ag, batches, on)[0].clone()}
    for held_out in (4242, 4243, 4244):
        for name, p in patches.items():
            plain = evaluate_patch(ag, batches, p, on)[0].tolist()
            moved = evaluate_patch(ag, batches, p, on, seed=held_out, transforms=True)[0].tolist()
            fmt = lambda v: ", ".join(f"{k} {x:.6f}" for k, x in zip(EVAL_KEYS, v))  # noqa: E731
            print(f"seed {held_out} {name:10s}: at the base offset {fmt(plain)} | transformed {fmt(moved)}", flush=True)


if __name__ == "__main__":
    if sys.argv[1] == "train":
        train(sys.argv[2] == "on", int(sys.argv[3]) if len(sys.argv) > 3 else 5)
    else:
        robust()
