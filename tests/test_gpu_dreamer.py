"""End-to-end parity of the HIP update path against the golden vectors of the real reference.

For each BASELINE config family (tests/golden/*.npz: proprio/dreamer, walker/r2dreamer, walker/dreamer-decoder,
atari-like discrete/32x32, memory-maze-like deter 4096) the product Dreamer is given the reference weights
(through load_state_dict, exercising the checkpoint layout), the same batch, initial latents and noise seed,
and runs two full updates (WM fwd+bwd, imagination, actor/critic, AGC+LaProp). Stated tolerances:
  * world-model losses (dyn, rep, rew, con, barlow / recon): <= 1e-4 relative (BASELINE.json north_star);
  * all other losses / metrics: <= 1e-3 relative (actor/critic terms sit behind sampled actions and sums over
    symexp bins up to 4.8e8);
  * posterior / imagined latent indices: bit-exact except near-ties (top-2 perturbed-logit margin < 1e-5);
  * parameters after each LaProp step: <= 2e-3 relative to the step size (LaProp normalises the gradient).
"""
import copy
import json
import os

import numpy as np
import pytest
import torch

from golden_io import CASES, batch, case_overrides, initial, load_case, sample_idx
from parity import assert_close, bound_ratio, compare_indices, imag_margins, post_margins, ulp
from sdreamer.config import load_config

pytestmark = pytest.mark.gpu
DEV = "cuda"
WM_KEYS = ("dyn", "rep", "rew", "con", "barlow", "infonce", "swav", "temp", "norm", "image", "position", "velocity")


class _Sp:
    def __init__(self, shape):
        self.shape = tuple(shape)


class _Spaces:
    def __init__(self, d):
        self.spaces = d


def build_agent(name):
    from sdreamer.dreamer import Dreamer
    z, cfg, spec, params, obs = load_case(name)
    cfg_name = CASES[name][0]
    H = int(z["meta_H"])
    gcfg = load_config(cfg_name, ["device=cuda:0", "model.compile=False", f"model.imag_horizon={H}"] +
                       case_overrides(name))
    act = _Sp((int(z["meta_A"]),))
    if bool(z["meta_discrete"]):
        act.discrete = True
    ag = Dreamer(copy.deepcopy(gcfg.model), _Spaces({k: _Sp(v) for k, v in obs.items()}), act)
    sd = {k: torch.from_numpy(v) for k, v in params.items()}
    for k, sk in list(spec.slow_names.items()) + list(spec.ema_names.items()):
        sd[sk] = torch.from_numpy(params[k])
    sd["return_ema.ema_vals"] = torch.zeros(2)
    missing, unexpected = ag.load_state_dict(sd, strict=False)
    assert not unexpected, unexpected
    assert not [m for m in missing if not m.startswith("_frozen")], missing
    return ag, z, spec, obs


def _rel(a, b):
    return abs(float(a) - float(b)) / max(abs(float(b)), 1e-6)


class _OracleRun:
    """Lazily runs the CPU oracle over the same two updates (only when a near-tie margin is needed)."""

    def __init__(self, name, z, spec, obs):
        self.name, self.z, self.spec, self.obs = name, z, spec, obs
        self.keeps = None

    def keep(self, u):
        if self.keeps is None:
            from oracle.ref_cpu import OracleAgent
            _, _, _, params, _ = load_case(self.name)
            orc = OracleAgent(self.spec, params)
            self.keeps = []
            for v in range(2):
                k = {}
                orc.update(batch(self.z, v, self.obs), initial(self.z, v, self.spec), int(self.z[f"u{v}_seed"]), keep=k)
                self.keeps.append(k)
        return self.keeps[u]


def _opt_samples(ag, spec):
    """name -> (exp_avg, exp_avg_sq) sampled like the golden u*_st_* (LaProp state index i = _named_params[i])."""
    sd = ag._optimizer.state_dict()["state"]
    sd_name = {id(p): n for n, p in ag.named_parameters()}  # _named_params keys can differ (prj vs projector)
    out = {}
    for i, prm in enumerate(ag._named_params.values()):
        k = sd_name[id(prm)]
        if k not in spec.shapes or i not in sd:
            continue
        m = sd[i]["exp_avg"].reshape(-1).cpu().numpy()
        v = sd[i]["exp_avg_sq"].reshape(-1).cpu().numpy()
        idx = sample_idx(k, m.size)
        out[k] = (m[idx], v[idx])
    return out


@pytest.mark.parametrize("name", list(CASES))
def test_update_matches_reference(name):
    ag, z, spec, obs = build_agent(name)
    orc = _OracleRun(name, z, spec, obs)
    SK, S, Kd = spec.SK, spec.S, spec.K
    unimix = float(spec.unimix)
    _, _, _, params0, _ = load_case(name)
    prev = {k: params0[k].reshape(-1)[sample_idx(k, params0[k].size)] for k in spec.shapes}
    report = {}
    bounds, bounds64 = {}, {}
    f64p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f64", f"{name}.npz")
    f64 = np.load(f64p) if os.path.exists(f64p) else None
    for u in range(2):
        seed = int(z[f"u{u}_seed"])
        data = batch(z, u, obs, DEV)
        if "image" in obs:
            data["image"] = torch.from_numpy(z[f"u{u}_in_image"]).to(DEV)  # uint8: exercise preprocess
        init = initial(z, u, spec, DEV)
        (ps, pd), mets = ag.update_batch(data, init, seed)
        torch.cuda.synchronize()
        # posterior latents (rssm.py:140-178): bit-exact except near-ties; deter / logits on the rows that did not flip
        ref_logit = z[f"u{u}_post_logit"]
        dv = compare_indices(ps.argmax(-1).cpu().numpy(), z[f"u{u}_post_idx"],
                             lambda: post_margins(ref_logit, seed, unimix), f"u{u} posterior indices")
        keep_rows = ~dv
        report[f"u{u}_post_flips"] = int(dv.sum())
        pdv = pd.detach().cpu().numpy()[..., ::4]
        assert_close(pdv, z[f"u{u}_post_deter"], 1e-4, 1e-5, f"u{u} post_deter", mask=~keep_rows[..., None])
        pl = ag._last["post_logit"].detach().cpu().numpy()
        assert_close(pl, ref_logit, 1e-4, 1e-4, f"u{u} post_logit", mask=~keep_rows[..., None, None])
        prl = ag._last["prior_logit"].detach().cpu().numpy().reshape(ref_logit.shape)
        assert_close(prl, z[f"u{u}_prior_logit"], 1e-4, 1e-4, f"u{u} prior_logit", mask=~keep_rows[..., None, None])
        report[f"u{u}_post_deter"] = float(np.abs(pdv - z[f"u{u}_post_deter"]).max())
        # imagination (dreamer.py:673-692): time-major (H+1, N, F) -> batch-major
        ifeat = ag._last["imag_feat_tm"].detach().transpose(0, 1).cpu().numpy()
        N, H1 = ifeat.shape[:2]
        iidx = ifeat[..., :SK].reshape(N, H1, S, Kd).argmax(-1)

        def imargin():
            k = orc.keep(u)
            m = imag_margins(k["imag_prior_logit"].numpy(), seed, unimix)
            return np.concatenate([np.full((N, 1, S), np.inf, np.float32), m], 1)  # feat 0 = posterior start

        start_bad = dv.reshape(-1)  # imagination starts from the posterior rows (b, t): a flipped start diverges
        idv = compare_indices(iidx, z[f"u{u}_imag_idx"], imargin, f"u{u} imagined indices")
        idv = idv | start_bad[:, None]
        report[f"u{u}_imag_flips"] = int(idv.sum())
        print(name, report, flush=True)  # (on a failure below, the flips so far)
        assert_close(ifeat[..., SK::16], z[f"u{u}_imag_deter"], 1e-4, 1e-5, f"u{u} imag_deter", mask=idv[..., None])
        iact = ag._last["imag_action_tm"].detach().transpose(0, 1).cpu().numpy()
        assert_close(iact, z[f"u{u}_imag_action"], 1e-4, 1e-5, f"u{u} imag_action", mask=idv[..., None])
        ret = ag._last["ret"].detach().cpu().numpy()[..., None]
        rows_ok = ~idv.any(1)
        assert_close(ret, z[f"u{u}_imag_ret"], 1e-3, 1e-4, f"u{u} imag_ret", mask=~rows_ok[:, None, None])
        rret = ag._last["rret"].detach().cpu().numpy()[..., None]
        if rows_ok.all():
            assert_close(rret, z[f"u{u}_replay_ret"], 1e-3, 1e-4, f"u{u} replay_ret")
            assert_close(ag.return_ema.ema_vals.cpu().numpy(), z[f"u{u}_ema_vals"], 1e-4, 1e-6, f"u{u} ema_vals")
        report[f"u{u}_imag_deter"] = float(np.where(idv[..., None], 0, np.abs(ifeat[..., SK::16] - z[f"u{u}_imag_deter"])).max())
        report[f"u{u}_ret"] = float(np.abs(ret - z[f"u{u}_imag_ret"]).max())
        # losses and metrics
        bad = []
        for k, v in mets.items():
            key = f"u{u}_m_{k}"
            if key not in z:
                continue
            tol = 1e-4 if (k.startswith("loss/") and k[5:] in WM_KEYS) else 1e-3
            if k.startswith("action_") or k.startswith("ret") or k in ("adv", "adv_std", "tar", "val", "rew",
                                                                         "slowval", "opt/loss") or \
                    k.startswith("value_replay") or k.startswith("slow_value_replay"):
                tol = 5e-3
            r = _rel(v, z[key])
            if r > tol and abs(float(v) - float(z[key])) > 1e-5:
                bad.append((k, float(v), float(z[key]), r))
        assert not bad, bad
        # LaProp moments and the parameter step (laprop.py:85-116 after agc.py:15-53), per sampled element.
        # v = EMA of (AGC-scaled g)^2 pins every gradient element's magnitude; m and dp carry its sign. Elements whose
        # gradient is ~0 relative to the tensor (|g| < 1e-3 of the sample max) may take either sign: excluded there.
        # Gradient elements carry the split-bf16 contraction error, amplified by cancellation in long sums (e.g. the
        # first conv layer's weight gradient sums dy*x over B*T*64*64 pixels: up to ~0.5 % of an element measured),
        # so v is held to 2e-2 rel + 2e-4 of max v, m and dp to 2e-2 rel + 1e-2 of their sample max (+ 4 ulp of p):
        # a flipped step sign (2x), a skipped AGC clip (1/scale^2 in v) or a skipped Polyak still fail
        # (tools/sabotage_optim.sh).
        opt = _opt_samples(ag, spec)
        # distance from the float64 run of the same update (tests/golden/gen_f64_moments.py), reported beside the
        # golden's bounds (tools/grad_attrib.py compares both f32 runs against it). Not asserted: where a term is
        # ill-conditioned the f64 run moves away from every f32 evaluation (walker_r2_nowarm: product and golden agree
        # to 0.004 of the bound and both sit 0.2 from f64), so it is evidence for attribution, not an oracle.
        if f64 is not None:
            for k in spec.shapes:
                m, v = opt[k]
                m64, v64 = f64[f"u{u}_{k}__m"], f64[f"u{u}_{k}__v"]
                tiny64 = np.sqrt(v64) < 1e-3 * np.sqrt(v64).max()
                for what, br in (("v", bound_ratio(v, v64, 2e-2, 2e-4 * np.abs(v64).max() + 1e-30)),
                                 ("m", bound_ratio(m, m64, 2e-2, 1e-2 * np.abs(m64).max() + 1e-30, mask=tiny64))):
                    if br > bounds64.get(what, ("", 0.0))[1]:
                        bounds64[what] = (k, br)
        if os.environ.get("SDREAMER_DUMP_OPT"):  # sampled LaProp moments, for tools/grad_attrib.py
            d = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "gpurun_out", "golden")
            os.makedirs(d, exist_ok=True)
            np.savez(os.path.join(d, f"{name}_opt_u{u}.npz"),
                     **{f"{k}__{w}": a for k, (m_, v_) in opt.items() for w, a in (("m", m_), ("v", v_))})
        sd = ag.state_dict()
        worst = 0.0
        for k in spec.shapes:
            m, v = opt[k]
            m_ref, v_ref = z[f"u{u}_st_{k}__m"], z[f"u{u}_st_{k}__v"]
            tiny = np.sqrt(v_ref) < 1e-3 * np.sqrt(v_ref).max()
            rv = bound_ratio(v, v_ref, 2e-2, 2e-4 * np.abs(v_ref).max() + 1e-30)
            rm = bound_ratio(m, m_ref, 2e-2, 1e-2 * np.abs(m_ref).max() + 1e-30, mask=tiny)
            exact = False
            if max(rv, rm) > 1 and f64 is not None:
                # The reference's f32 answer OR exact arithmetic, on the same bounds: where a
                # moment is ill-conditioned the reference's own f32 sits far from the float64 run of the same update
                # (walker_r2_nowarm's first conv layer: 5.1 of the bound), and a kernel whose rounding differs from
                # the reference's can land next to the float64 answer instead (the bf16x6 encoder: 0.02). Either is
                # a correct evaluation of the reference's update; anything else still fails.
                m64, v64 = f64[f"u{u}_{k}__m"], f64[f"u{u}_{k}__v"]
                tiny64 = np.sqrt(v64) < 1e-3 * np.sqrt(v64).max()
                rv64 = bound_ratio(v, v64, 2e-2, 2e-4 * np.abs(v64).max() + 1e-30)
                rm64 = bound_ratio(m, m64, 2e-2, 1e-2 * np.abs(m64).max() + 1e-30, mask=tiny64)
                assert max(rv64, rm64) <= 1, (f"u{u} moments {k}: {rv:.3g} / {rm:.3g} of the golden's bound (v / m), "
                                              f"{rv64:.3g} / {rm64:.3g} of the float64 run's")
                report.setdefault("exact_arithmetic", []).append((u, k, rv, rm, rv64, rm64))
                exact = True
            else:
                assert_close(v, v_ref, 2e-2, 2e-4 * np.abs(v_ref).max() + 1e-30, f"u{u} exp_avg_sq {k}")
                assert_close(m, m_ref, 2e-2, 1e-2 * np.abs(m_ref).max() + 1e-30, f"u{u} exp_avg {k}", mask=tiny)
            for what, br in (("v", rv), ("m", rm)):
                if br > bounds.get(what, ("", 0.0))[1] and not exact:
                    bounds[what] = (k, br)
            flat = sd[k].detach().reshape(-1).cpu().numpy()
            got = flat[sample_idx(k, flat.size)]
            ref = z[f"u{u}_p_{k}__s"]
            d_got, d_ref = got.astype(np.float64) - prev[k], ref.astype(np.float64) - prev[k]
            if not exact:  # (the float64 fixture holds moments only; the step follows from them)
                assert_close(d_got, d_ref, 2e-2, 1e-2 * np.abs(d_ref).max() + 4 * ulp(ref),
                             f"u{u} parameter step {k}", mask=tiny)
            br = bound_ratio(d_got, d_ref, 2e-2, 1e-2 * np.abs(d_ref).max() + 4 * ulp(ref), mask=tiny)
            if br > bounds.get("step", ("", 0.0))[1]:
                bounds["step"] = (k, br)
            nz_ = (~tiny) & (np.abs(d_ref) > 0)
            if nz_.any():
                worst = max(worst, float((np.abs(d_got - d_ref)[nz_] / np.abs(d_ref)[nz_]).max()))
            prev[k] = ref.astype(np.float64)
        report[f"u{u}_max_rel_dp"] = worst
        # slow critic after this update's Polyak (dreamer.py:242-249): s = 0.02 v + 0.98 s, before the step
        for k, sk in spec.slow_names.items():
            flat = sd[sk].detach().reshape(-1).cpu().numpy()
            ref = z[f"u{u}_p_{sk}__s"]
            assert_close(flat[sample_idx(sk, flat.size)], ref, 0.0, 4 * ulp(ref) + 1e-12, f"u{u} slow critic {sk}")
    report["bound_ratio"] = {k: {"tensor": t, "ratio": r} for k, (t, r) in bounds.items()}
    report["bound_ratio_f64"] = {k: {"tensor": t, "ratio": r} for k, (t, r) in bounds64.items()}
    print(name, report)
    if not os.environ.get("SDREAMER_GOLDEN_REPORT"):  # opt-in file report (set by one-off drivers, removed)
        return
    out = os.environ["SDREAMER_GOLDEN_REPORT"]
    os.makedirs(out, exist_ok=True)
    with open(os.path.join(out, f"{name}{'_f32' if os.environ.get('SDREAMER_FAST_GEMM') == '0' else ''}.json"),
              "w") as f:
        json.dump(report, f, indent=1, sort_keys=True)


@pytest.mark.parametrize("name", ["walker_r2", "walker_r2aug", "walker_pro"])
def test_graph_replay_matches_eager(name):
    """HIP-graph replays (update 3+) produce exactly the eager results: same kernels, device-resident seed
    (walker_r2aug: the augmentation shifts also follow the device seed)."""
    runs = []
    for graphs in (False, True):
        ag, z, spec, obs = build_agent(name)
        ag.use_graphs = graphs
        out = []
        for u in range(5):
            data = batch(z, u % 2, obs, DEV)
            init = initial(z, u % 2, spec, DEV)
            (ps, pd), mets = ag.update_batch(data, init, 500 + u)
            out.append((float(mets["loss/dyn"]), float(mets["loss/value"]), float(mets["opt/loss"]),
                        pd.detach().clone(), ps.argmax(-1).clone()))
        sd = ag.state_dict()
        out.append(torch.cat([sd[k].reshape(-1) for k in spec.shapes]).clone())
        runs.append(out)
    (e, g) = runs
    assert ag._graph is not None
    for u in range(5):
        assert e[u][:3] == g[u][:3], (u, e[u][:3], g[u][:3])
        assert torch.equal(e[u][3], g[u][3]) and torch.equal(e[u][4], g[u][4])
    assert torch.equal(e[5], g[5])


@pytest.mark.parametrize("name", list(CASES))
def test_cal_grad_matches_reference(name):
    """Gradients of one _cal_grad at the initial weights vs the reference's (golden g_*: per-tensor L2 norm and 32
    sampled elements of every trainable tensor). walker_pro checks the prototype / projection gradients that the
    default prototype freeze zeroes before the optimizer step. Gradient contractions run split-bf16:
    elements within 2e-3 relative + 1e-4 of the tensor's largest sampled |g|; norms within 2e-4 — of the reference's
    f32 gradient, or of the float64 gradient of the same _cal_grad (tests/golden/f64) where the reference's own f32
    is farther than that from exact arithmetic."""
    ag, z, spec, obs = build_agent(name)
    ag.use_graphs = False
    data = ag.preprocess(batch(z, 0, obs, DEV))
    init = initial(z, 0, spec, DEV)
    ag._update_slow_target()
    if spec.rep_loss == "dreamerpro":
        ag.ema_update()
    ag._optimizer.zero_grad()
    ag._cal_grad(data, init, 1000, 0)
    torch.cuda.synchronize()
    named = dict(ag.named_parameters())
    f64p = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "f64", f"{name}.npz")
    f64 = np.load(f64p) if os.path.exists(f64p) else None

    def check(flat, ref_n, ref):
        """(failures, worst element rel err) of one gradient against one answer (norm, sampled elements)"""
        out = []
        n = float(np.linalg.norm(flat))
        if abs(n - ref_n) > 2e-4 * max(ref_n, 1e-9) and abs(n - ref_n) > 1e-9:
            out.append(("norm", n, ref_n))
        got = flat[sample_idx(k, flat.size)]
        scale = np.abs(ref).max()
        err = np.abs(got - ref) - (2e-3 * np.abs(ref) + 1e-4 * scale + 1e-12)
        if err.max() > 0:
            i = int(np.argmax(err))
            out.append(("element", float(got[i]), float(ref[i])))
        return out, float((np.abs(got - ref) / (np.abs(ref) + 1e-3 * scale + 1e-30)).max())

    bad, worst, exact = [], (0.0, None), []
    for k in spec.shapes:
        g = named[k].grad
        g = torch.zeros_like(named[k]) if g is None else g
        flat = ag.to_ref_layout(named[k], g).reshape(-1).double().cpu().numpy()
        fails, r = check(flat, float(z[f"g_{k}__n"]), z[f"g_{k}__s"].astype(np.float64))
        if fails and f64 is not None and f"g_{k}__s" in f64.files:
            # the reference's f32 gradient OR the exact-arithmetic one (tests/golden/f64, the oracle's float64
            # cal_grad), on the same bounds: walker_r2_nowarm's encoder gradients are ill-conditioned — the
            # reference's own f32 sits 6.3 of this bound from float64 — and the bf16x6 encoder lands next to float64
            fails64, r64 = check(flat, float(f64[f"g_{k}__n"]), f64[f"g_{k}__s"])
            if not fails64:
                exact.append((k, round(r, 4), round(r64, 4)))
                fails, r = [], r64
        bad += [(k,) + f for f in fails]
        if r > worst[0]:
            worst = (r, k)
    print(name, "worst element rel err", worst, "| tensors matching the float64 gradient instead:", exact)
    assert not bad, bad


@pytest.mark.parametrize("name", ["walker_r2", "walker_dreamer", "proprio_dreamer", "atari_r2", "maze_r2"])
def test_weight_init_matches_reference(name):
    """Dreamer's own initialisation (networks._trunc_normal_ = tools.weight_init_, tools.py:76-100, plus the
    outscale of the last head layers, networks.py:370-372) vs the reference's initialiser run under
    torch.manual_seed(0) (golden init_*__stat: mean, std, max|w|, numel per tensor). The draws differ (different
    RNG call order), so the test is distributional: constants (zero biases, unit norm scales, outscale 0) exact;
    std within 4/sqrt(n) + 1 %, mean within 6 std/sqrt(n), max|w| <= 2 sigma (the truncation) and >= 0.5x the
    reference's (the 2 sigma bound is taken from the reference's sample std, widened by its sampling error)."""
    from sdreamer.dreamer import Dreamer
    z, cfg, spec, params, obs = load_case(name)
    gcfg = load_config(CASES[name][0], ["device=cuda:0", "model.compile=False"] + case_overrides(name))
    act = _Sp((int(z["meta_A"]),))
    if bool(z["meta_discrete"]):
        act.discrete = True
    torch.manual_seed(0)
    ag = Dreamer(copy.deepcopy(gcfg.model), _Spaces({k: _Sp(v) for k, v in obs.items()}), act)
    sd = ag.state_dict()
    bad = []
    for k in spec.shapes:
        mean_r, std_r, amax_r, n = (float(x) for x in z[f"init_{k}__stat"])
        w = sd[k].detach().double().reshape(-1).cpu()
        assert w.numel() == int(n), k
        mean, std, amax = w.mean().item(), (w.std().item() if w.numel() > 1 else 0.0), w.abs().max().item()
        if std_r == 0.0:
            if not (mean == mean_r and amax == amax_r):
                bad.append((k, "constant", mean, mean_r))
            continue
        sigma = std_r / 0.8796  # std of N(0, s^2) truncated at +-2s is 0.8796 s
        if abs(std / std_r - 1) > 4 / np.sqrt(n) + 0.01:
            bad.append((k, "std", std, std_r))
        if abs(mean - mean_r) > 6 * std_r / np.sqrt(n):
            bad.append((k, "mean", mean, mean_r))
        if amax > max(2 * sigma * (1 + 4 / np.sqrt(n)), amax_r) * 1.001 or amax < 0.5 * amax_r:
            bad.append((k, "max", amax, amax_r))
    assert not bad, bad


def test_pair_first_matches_per_head():
    """ops.PairFirstFn (the imagined actor's and value head's first-layer weight gradients as one GEMM over their
    joint dy, their weights back to back in the arena) against the per-head path on the same agent, at the bench's
    full C2 size (H * N = 15,360 rows: the joint GEMM runs; at the golden sizes it falls back to per-head GEMMs): every
    gradient outside those two layers' weights / biases bit-identical, those within the split-bf16 bound."""
    from fullsize_io import FULL, OVERRIDES, PARAM_SEED, SEED, full_inputs
    from oracle.init import params_for
    from oracle.ref_cpu import Spec
    from sdreamer.dreamer import Dreamer
    name = "C2_walker_r2"
    cfg_name, ovr, obs, A, discrete, B, L, H = FULL[name]
    gcfg = load_config(cfg_name, ["device=cuda:0"] + ovr + OVERRIDES)
    spec = Spec(gcfg.model, obs, A, discrete)
    ag = Dreamer(copy.deepcopy(gcfg.model), _Spaces({k: _Sp(v) for k, v in obs.items()}), _Sp((A,)))
    sd = {k: torch.from_numpy(v) for k, v in params_for(spec.shapes, PARAM_SEED).items()}
    ag.load_state_dict(sd, strict=False)
    assert ag._pair_first
    ag.use_graphs = False
    data_np, init_np = full_inputs(name, spec.K, spec.S, spec.D)
    data = ag.preprocess({k: torch.from_numpy(v).cuda() for k, v in data_np.items()})
    init = tuple(torch.from_numpy(v).cuda() for v in init_np)
    ag._update_slow_target()
    grads = []
    for pair in (True, False):
        ag._pair_first = pair
        ag._optimizer.zero_grad()
        ag._cal_grad(data, init, SEED, 0)
        torch.cuda.synchronize()
        grads.append({n: p.grad.detach().clone() for n, p in ag._named_params.items()})
    first = {id(ag.actor.mlp._mods[0][0].weight), id(ag.actor.mlp._mods[0][0].bias),
             id(ag.value.mlp._mods[0][0].weight), id(ag.value.mlp._mods[0][0].bias)}
    checked = 0
    for n, p in ag._named_params.items():
        a, b = grads[0][n], grads[1][n]
        if id(p) in first:
            scale = float(b.abs().max())
            assert float((a - b).abs().max()) <= 2e-3 * scale + 1e-12, (n, float((a - b).abs().max()), scale)
            checked += 1
        else:
            assert torch.equal(a, b), n
    assert checked == 4

