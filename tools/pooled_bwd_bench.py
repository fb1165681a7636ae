"""Encoder stages 2 and 3 backward at the bench's 1,024 images, each launch alone, on both routes: the max-pool backward
(full-resolution scatter / pooled-resolution), the split-bf16 bwd-weight and bwd-data from the full-resolution conv
gradient and from (dpool, argmax). Median of N launches by HIP events, in us, and the two results compared bit for bit.

Usage: python tools/pooled_bwd_bench.py [N=30] [images=1024]   (N = 1 under rocprofv3 --pmc: one dispatch per kernel)"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "safe-dreamer_amd"))
import torch  # noqa: E402

from sdreamer import kernels as K  # noqa: E402


def timeit(fn, n):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return sorted(ts)[len(ts) // 2]


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 30
    nb = int(sys.argv[2]) if len(sys.argv) > 2 else 1024
    g = torch.Generator().manual_seed(0)
    for ci, co, hw in ((32, 48, 32), (48, 64, 16)):
        x = torch.randn(nb, hw, hw, ci, generator=g).cuda()
        w = (torch.randn(co, 5, 5, ci, generator=g) / (25 * ci) ** 0.5).cuda()
        b, nw = torch.zeros(co).cuda(), torch.ones(co).cuda()
        _, pooled, amax, rstd = K.conv2d_fwd_pool(x, w, b, nw)
        dy = torch.randn(pooled.shape, generator=g).cuda()
        K.set_flip_cache([w])
        out = {}

        def full():
            out["dconv"] = K.pool_rms_bwd(pooled, amax, nw, rstd, dy, hw, hw, torch.zeros_like(nw))

        def compact():
            out["dpool"] = K.pool_rms_bwd_compact(pooled, amax, nw, rstd, dy, torch.zeros_like(nw))

        t = {"pool_rms_bwd": (timeit(full, n), timeit(compact, n))}
        dconv, dpool = out["dconv"], out["dpool"]
        t["bwd-weight"] = (timeit(lambda: out.__setitem__("dw", K.conv2d_wgrad(x, dconv, 5, 5)), n),
                           timeit(lambda: out.__setitem__("dwp", K.conv2d_wgrad_pooled(x, dpool, amax, 5, 5)), n))
        t["bwd-data"] = (timeit(lambda: out.__setitem__("dx", K.conv2d_dgrad(dconv, w)), n),
                         timeit(lambda: out.__setitem__("dxp", K.conv2d_dgrad_pooled(dpool, amax, w)), n))
        same = torch.equal(out["dw"], out["dwp"]) and torch.equal(out["dx"], out["dxp"])
        print(f"stage {ci} -> {co} at {hw} x {hw}, {nb} images (us, full resolution -> pooled; results bit-identical: {same})")
        for k, (a, c) in t.items():
            print(f"  {k:13s} {a:8.1f} -> {c:8.1f}")
        print(f"  {'sum':13s} {sum(a for a, _ in t.values()):8.1f} -> {sum(c for _, c in t.values()):8.1f}")
        K.clear_flip_cache()


if __name__ == "__main__":
    main()
