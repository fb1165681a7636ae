"""Timings of the wide conv encoder (a stage width above 128 channels; profiles/wide_encoder.md holds the results).

  kernels  the two wide split-bf16 backward contractions (sd_conv2d_dgrad_wide3 / sd_conv2d_wgrad_wide3) against the
           exact-f32 generic tiles the same calls run with fast=False, at the depth-77 stage shapes and --nb images:
           device events, warmed, --rounds rounds alternating old and new arm. Per shape: microseconds, TFLOP/s from
           the shape's 2 M N K, the share of the bf16x3 ceiling, and whether the new arm's slowest round beats the f32
           arm's fastest.
  rows     the wide pool / RMSNorm / SiLU row kernels at the stage-1 and stage-2 sizes (microseconds, bytes/s against
           HBM peak), and C = 128 through the narrow kernel next to C = 129 through the wide one.
  update   one depth-77 update (dmc/wider_cnn) at --batch x --length, eager and graphed: ms per update, the encoder's
           forward and backward alone, the rest, peak memory.

  python tools/wide_encoder_bench.py kernels rows update [--nb 1024] [--out FILE.json]
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "safe-dreamer_amd")]

import torch  # noqa: E402

DEV = "cuda"
BF16_DENSE_TFLOPS = 2516.6  # MI355X bf16 MFMA peak; the split path issues three MFMAs per product
X3_CEILING = BF16_DENSE_TFLOPS / 3
HBM_GBS = 8000.0
# depth 77: (Ci, Co, H = W) of the four stages' convolutions (the first on the channel-padded image)
STAGES = [("s1 4->154 @64", 4, 154, 64), ("s2 154->231 @32", 154, 231, 32), ("s3 231->308 @16", 231, 308, 16),
          ("s4 308->308 @8", 308, 308, 8)]


def timed(fn, reps):
    """median microseconds of fn() over reps runs, each between two device events"""
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    for s, e in ev:
        s.record()
        fn()
        e.record()
    torch.cuda.synchronize()
    us = sorted(s.elapsed_time(e) * 1e3 for s, e in ev)
    return us[len(us) // 2]


def bench_kernels(nb, rounds, reps):
    from sdreamer import kernels as K
    out = []
    for label, ci, co, hw in STAGES:
        g = torch.Generator(device=DEV).manual_seed(hw)
        x = torch.randn(nb, hw, hw, ci, device=DEV, generator=g)
        dout = torch.randn(nb, hw, hw, co, device=DEV, generator=g)
        w = torch.randn(co, 5, 5, ci, device=DEV, generator=g) / (25 * ci) ** 0.5
        K.set_flip_cache([w])
        flops = 2.0 * nb * hw * hw * co * 25 * ci
        ops = {"dgrad": lambda fast: K.conv2d_dgrad(dout, w, fast=fast),
               "wgrad": lambda fast: K.conv2d_wgrad(x, dout, 5, 5, fast=fast)}
        for op, fn in ops.items():
            for fast in (False, True):  # warm-up (and the allocator's blocks)
                fn(fast)
            torch.cuda.synchronize()
            old, new = [], []
            for _ in range(rounds):
                old.append(timed(lambda: fn(False), reps))
                new.append(timed(lambda: fn(True), reps))
            row = dict(shape=label, op=op, nb=nb, f32_us=old, x3_us=new, f32_tflops=flops / min(old) / 1e6,
                       x3_tflops=flops / min(new) / 1e6, x3_ceiling_share=flops / min(new) / 1e6 / X3_CEILING,
                       speedup=min(old) / min(new), accepted=max(new) < min(old))
            out.append(row)
            print(json.dumps(row), flush=True)
        K.clear_flip_cache()
        del x, dout, w
        torch.cuda.empty_cache()
    return out


def bench_rows(nb, reps):
    from sdreamer import kernels as K
    out = []
    for label, C, hw, wide in (("s1 C=154 @64", 154, 64, True), ("s2 C=231 @32", 231, 32, True),
                               ("narrow C=128 @64", 128, 64, False), ("wide C=129 @64", 129, 64, True)):
        g = torch.Generator(device=DEV).manual_seed(C)
        x = torch.randn(nb, hw, hw, C, device=DEV, generator=g)
        nw = torch.ones(C, device=DEV)
        fwd, bwd = (K.pool_rms_wide_fwd, K.pool_rms_wide_bwd) if wide else (K.pool_rms_fwd, K.pool_rms_bwd)
        y, pooled, amax, rstd = fwd(x, nw)
        dy = torch.randn_like(y)
        dnw = torch.zeros(C, device=DEV)
        bwd(pooled, amax, nw, rstd, dy, hw, hw, dnw)
        torch.cuda.synchronize()
        n, p = x.numel(), pooled.numel()
        f_us = timed(lambda: fwd(x, nw), reps)
        b_us = timed(lambda: bwd(pooled, amax, nw, rstd, dy, hw, hw, dnw), reps)
        f_bytes, b_bytes = 4 * n + 9 * p, 4 * n + 9 * p  # x | pooled, y, amax   and   dx | pooled, dy, amax
        row = dict(shape=label, nb=nb, fwd_us=f_us, bwd_us=b_us, fwd_gbs=f_bytes / f_us / 1e3,
                   bwd_gbs=b_bytes / b_us / 1e3, fwd_hbm_share=f_bytes / f_us / 1e3 / HBM_GBS,
                   bwd_hbm_share=b_bytes / b_us / 1e3 / HBM_GBS)
        out.append(row)
        print(json.dumps(row), flush=True)
        del x, y, pooled, amax, rstd, dy
        torch.cuda.empty_cache()
    return out


class _Sp:
    def __init__(self, shape):
        self.shape = tuple(shape)


class _Spaces:
    def __init__(self, d):
        self.spaces = d


def bench_update(B, L, H, steps):
    from sdreamer.config import load_config
    from sdreamer.dreamer import Dreamer
    cfg = load_config("dmc/wider_cnn", ["device=cuda:0", "model.compile=False", f"model.imag_horizon={H}"])
    out = {}
    g = torch.Generator().manual_seed(0)
    data = dict(image=torch.randint(0, 256, (B, L, 64, 64, 3), dtype=torch.uint8, generator=g),
                action=torch.rand(B, L, 6, generator=g) * 2 - 1, reward=torch.rand(B, L, 1, generator=g),
                is_first=torch.zeros(B, L, 1, dtype=torch.bool), is_terminal=torch.zeros(B, L, 1, dtype=torch.bool),
                is_last=torch.zeros(B, L, 1, dtype=torch.bool))
    data["is_first"][:, 0] = True
    data = {k: v.to(DEV) for k, v in data.items()}
    for mode in ("eager", "graphed"):
        torch.manual_seed(0)
        ag = Dreamer(copy.deepcopy(cfg.model), _Spaces({"image": _Sp((64, 64, 3))}), _Sp((6,)))
        ag.use_graphs = mode == "graphed"
        init = ag.get_initial_state(B)
        init = (init["stoch"], init["deter"]) if isinstance(init, dict) else init
        torch.cuda.reset_peak_memory_stats()
        for i in range(3):
            ag.update_batch(data, init, 100 + i)
        torch.cuda.synchronize()
        ms = []
        for i in range(steps):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            ag.update_batch(data, init, 200 + i)
            e.record()
            torch.cuda.synchronize()
            ms.append(s.elapsed_time(e))
        out[mode] = dict(ms=sorted(ms)[len(ms) // 2], all_ms=ms, peak_gib=torch.cuda.max_memory_allocated() / 2 ** 30)
        print(json.dumps({mode: out[mode]}), flush=True)
        if mode == "eager":  # the encoder alone: forward, then backward from a random gradient of the embedding
            pre = ag.preprocess(data)
            emb = ag._encode(pre)
            emb = emb[0] if isinstance(emb, (tuple, list)) else emb
            dy = torch.randn_like(emb)
            torch.cuda.synchronize()

            def fwd():
                e2 = ag._encode(pre)
                return e2[0] if isinstance(e2, (tuple, list)) else e2

            f_us = timed(lambda: fwd(), 5)
            both = timed(lambda: fwd().backward(dy), 5)
            out["encoder"] = dict(fwd_ms=f_us / 1e3, bwd_ms=(both - f_us) / 1e3)
            out["encoder"]["rest_ms"] = out["eager"]["ms"] - both / 1e3
            print(json.dumps({"encoder": out["encoder"]}), flush=True)
            ag._optimizer.zero_grad()
        del ag
        torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("what", nargs="+", choices=["kernels", "rows", "update"])
    ap.add_argument("--nb", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--length", type=int, default=64)
    ap.add_argument("--horizon", type=int, default=15)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if "kernels" in a.what:
        res["kernels"] = bench_kernels(a.nb, a.rounds, a.reps)
    if "rows" in a.what:
        res["rows"] = bench_rows(a.nb, a.reps)
    if "update" in a.what:
        res["update"] = bench_update(a.batch, a.length, a.horizon, a.steps)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
