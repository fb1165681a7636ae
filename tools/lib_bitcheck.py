"""Bit-identity check between two builds of libsdhip.so (A/B aid): computes the split-bf16 and f32 conv bwd-weight, the
pooled-gradient bwd-weight on both, the split-bf16 bwd-data, every output of the distribution-head kernels (csrc/dist.hip)
over the case tables of tests/rowop_models.py, every output of the pool / RMSNorm row entries (csrc/poolnorm.hip) at
each of their dispatch arms, every output of the dense contractions (csrc/gemm.hip, csrc/gemm3.hip: f32, split-bf16, weight
gradient, MLP and 256-wide MLP entries) over the case tables of tests/gemm_models.py, the fused imagination of the bench agent (random init, seed 0) and the
parameters after two eager updates of that agent on the bench's synthetic buffer, on fixed inputs, with the library
SDHIP_LIB points at, and saves them to argv[1]; `python tools/lib_bitcheck.py cmp a.npz b.npz` reports whether every array is bit-identical."""
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "safe-dreamer_amd"), os.path.join(ROOT, "tests")]


def rowops(res):
    """every array the float64 tests of csrc/dist.hip look at, over their full case tables (each dispatch arm)"""
    import rowop_models as rm
    import test_gpu_rowops_f64 as t
    for fam, fn, cases in (("sample", t.run_sample, rm.TEAM_CASES), ("logp", t.run_logp, rm.TEAM_CASES),
                           ("kl", lambda c: t.run_kl(c)[0], rm.KL_CASES), ("twohot", t.run_twohot, rm.TWOHOT_CASES),
                           ("repval", t.run_repval, rm.REPVAL_CASES), ("imag_ac", t.run_imag_ac, rm.IMAG_AC_CASES),
                           ("bnormal", t.run_bnormal, rm.BN_CASES), ("bernoulli", t.run_bernoulli, rm.BERN_ROWS),
                           ("gru", t.run_gru, rm.GRU_CASES)):
        for c in cases:
            for k, v in fn(c).items():
                res[f"{fam}/{getattr(c, 'name', c)}/{k}"] = v
    # the bounded normal's sampler and its backward, which no run_* above launches (test_gpu_imag_return_kernels.py)
    import torch
    import test_gpu_imag_return_kernels as ir
    from sdreamer import kernels as K
    for rows, A in ((1, 1), (65, 6), (65, 16)):
        x, d_an, _ = ir._bn_inputs(rows, A)
        xd, act = x.cuda(), torch.empty(rows, A, device="cuda")
        args = (ir.MIN_STD, ir.MAX_STD, ir.BN_SEED, ir.nz.STREAM_ACT, ir.BN_STEP, ir.BN_ROW_OFFSET)
        K.nat.call("sd_bnormal_sample", K.p(xd), K.p(act), rows, A, *args, 0, K.stream())
        res[f"bnormal_sample/{rows}x{A}/action"] = act.cpu().numpy()
        res[f"bnormal_sample/{rows}x{A}/dx"] = K.bnormal_sample_bwd(d_an.cuda(), xd, act, *args).cpu().numpy()


def rows(res):
    """every output of the pool / RMSNorm row entries (csrc/poolnorm.hip) through their kernels.py wrappers, at the
    smallest shape that reaches each arm: narrow C 9 / 32 / 48 / 128 (1 / 2 / 4 / 8 channels per lane), wide C 154 / 308
    (4 / 8), plain and FiLM (ipc 2), both output layouts, forward, backward and (narrow) the compact backward"""
    import torch
    from sdreamer import kernels as K
    for C in (9, 32, 48, 128, 154, 308):
        wide = C > K.WIDE_ROWS_MIN
        fwd, bwd = (K.pool_rms_wide_fwd, K.pool_rms_wide_bwd) if wide else (K.pool_rms_fwd, K.pool_rms_bwd)
        for Nb, H, W in ((4, 6, 6), (4, 5, 7)):
            g = torch.Generator().manual_seed(1000 * C + 10 * H + W)
            x = torch.randn(Nb, H, W, C, generator=g).cuda()
            w = (1 + 0.1 * torch.randn(C, generator=g)).cuda()
            film = ((1 + 0.2 * torch.randn(Nb // 2, C, generator=g)).cuda(),
                    (0.2 * torch.randn(Nb // 2, C, generator=g)).cuda())
            dy = torch.randn(Nb, H // 2, W // 2, C, generator=g)
            for fl in (None, film):
                for flat in (False, True):
                    key = f"rows/C{C}_{H}x{W}_{'film' if fl else 'plain'}_{'nchw' if flat else 'nhwc'}"
                    y, pooled, amax, rstd = fwd(x, w, nchw_flat=flat, film=fl)
                    d = (dy.permute(0, 3, 1, 2).reshape(Nb, -1) if flat else dy).contiguous().cuda()
                    outs = {"y": y, "pooled": pooled, "amax": amax, "rstd": rstd}
                    forms = [("bwd", lambda dw: bwd(pooled, amax, w, rstd, d, H, W, dw, nchw_flat=flat, film=fl))]
                    if not wide:
                        forms.append(("compact", lambda dw: K.pool_rms_bwd_compact(pooled, amax, w, rstd, d, dw,
                                                                                   nchw_flat=flat, film=fl)))
                    for name, call in forms:
                        dw = torch.zeros(C, device="cuda")
                        r = call(dw)
                        outs[f"{name}_dw"] = dw
                        for k, v in zip(("grad", "dgamma", "dbeta"), r if fl else (r,)):
                            outs[f"{name}_{k}"] = v
                    for k, v in outs.items():
                        res[f"{key}/{k}"] = v.cpu().numpy()


def gemms(res):
    """every output of the float64 tests of the dense contractions, over their full case tables (each dispatch arm):
    C, the row sums and part_out, as gemm/<family>/<case>/<output>; the N = 64 * odd part_out cases carry "po1" and an
    odd N / 64 in their names"""
    import gemm_models as gm
    import test_gpu_gemm_f64 as t
    for fam, cases in gm.CASES.items():
        for c in cases:
            for k, v in t.run(c)[0].items():
                if k == "pout_own":
                    continue
                v = v.astype(np.float32)
                if v.size > 1 << 20:  # the 256-wide cases' 50 MB outputs: their SHA-256
                    v = np.frombuffer(hashlib.sha256(v.tobytes()).digest(), np.uint8)
                res[f"gemm/{fam}/{c.name}/{k}"] = v


def run(out):
    import torch
    from sdreamer import kernels as K
    res = {}
    rowops(res)
    rows(res)
    gemms(res)
    for ci, co, hw, nb in [(32, 48, 32, 64), (48, 64, 16, 64), (64, 64, 8, 64), (4, 32, 64, 8)]:
        g = torch.Generator().manual_seed(ci * 7 + co)
        x = (torch.rand(nb, hw, hw, ci, generator=g) - 0.5).cuda()
        dy = torch.randn(nb, hw, hw, co, generator=g).cuda()
        w = (torch.randn(co, 5, 5, ci, generator=g) / (ci * 25) ** 0.5).cuda()
        res[f"dw_{ci}_{co}"] = K.conv2d_wgrad(x, dy, 5, 5, fast=True).cpu().numpy()
        res[f"dw_f32_{ci}_{co}"] = K.conv2d_wgrad(x, dy, 5, 5, fast=False).cpu().numpy()
        res[f"dx_{ci}_{co}"] = K.conv2d_dgrad(dy, w, fast=True).cpu().numpy()
    # the first stage's pooled-gradient bwd-weight (the loop's last shape: 4 -> 32 at 64 x 64, 8 images) on the
    # split-bf16 and on the f32 kernel
    dpool = torch.randn(nb, hw // 2, hw // 2, co, generator=g).cuda()
    amax = torch.randint(0, 4, dpool.shape, generator=g).to(torch.uint8).cuda()
    x3_default = K.WGRAD1_X3
    for x3 in (True, False):
        K.WGRAD1_X3 = x3
        res[f"dw_pool_x3_{int(x3)}"] = K.conv2d_wgrad_pool(x, dpool, amax, 5, 5).cpu().numpy()
    K.WGRAD1_X3 = x3_default
    import bench
    from sdreamer.config import load_config
    from sdreamer.dreamer import Dreamer
    cfg = load_config("dmc/cnn", ["device=cuda:0", "model.compile=False"])
    torch.manual_seed(0)
    ag = Dreamer(cfg.model, bench._Spaces({"image": bench._Sp((64, 64, 3))}), bench._Sp((6,)))
    g = torch.Generator().manual_seed(3)
    N, S, Kd, D = 1024, ag.rssm._stoch, ag.rssm._discrete, ag.rssm._deter
    stoch = torch.nn.functional.one_hot(torch.randint(0, Kd, (N, S), generator=g), Kd).float().cuda()
    deter = (0.5 * torch.randn(N, D, generator=g)).cuda()
    f, a = ag._imagine_tm((stoch, deter), 16, seed=77, row_offset=0)
    torch.cuda.synchronize()
    res["imag_feat"], res["imag_act"] = f.cpu().numpy(), a.cpu().numpy()
    # two eager updates (scan, encoder, heads, imagination, optimizer) on the bench's synthetic buffer
    L = int(cfg.batch_length)
    buf = bench.synth_buffer(cfg, torch.device("cuda", 0), 0, T=max(160, 2 * (L + 1)), A=6, discrete=False)
    for _ in range(2):
        ag.update(buf)
    torch.cuda.synchronize()
    res["update_params"] = ag._optimizer.arena.data.detach().cpu().numpy()
    np.savez(out, **res)


def cmp(a, b):
    za, zb = np.load(a), np.load(b)
    ok = True
    for k in za.files:
        same = za[k].shape == zb[k].shape and za[k].dtype == zb[k].dtype and za[k].tobytes() == zb[k].tobytes()
        diff = np.abs(za[k].astype(np.float64) - zb[k]).max() if za[k].shape == zb[k].shape else float("nan")
        print(f"{k}: {'bit-identical' if same else 'DIFFERENT max abs %.3g' % diff}")
        ok &= same
    print("ALL BIT-IDENTICAL" if ok else "MISMATCH")
    return 0 if ok else 1


if __name__ == "__main__":
    if sys.argv[1] == "cmp":
        sys.exit(cmp(sys.argv[2], sys.argv[3]))
    run(sys.argv[1])
