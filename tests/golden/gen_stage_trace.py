"""The launch trace of the conv encoder stage (fixture generator, needs the GPU; test infrastructure).

Records, through tests/launch_trace.py, every C-ABI launch the Python layer over the stage kernels issues (ops.py's
stage function, the kernels.py wrappers under it, the encoders' stage loops) for three groups of cases:

  stage/<name>    every conv_models.STAGE_CASES row, forward + backward, inputs as tests/test_gpu_conv_f64.py forms them
  switch/<...>    the two anchors of tests/test_gpu_conv_pooled_bwd.py (Nb 2), plain and FiLM, dx on and off, with one
                  of ops.POOL_COMPACT / ops.FUSED_POOL / K.CONV6 / K.WGRAD1_X3 off at a time
  update/<...>    walker_r2 and walker_mm_r2 (B2 T6): one eager update_batch and one observation_grad, each after one
                  warm-up call (the deferred bwd-weight queue, the first stage's split backward, the FiLM generators)

A refactor of that layer that leaves the trace as it is launches the same kernels with the same arguments in the same
order: same bits, same captured graph. tests/test_gpu_stage_trace.py replays the cases against the committed file, so
regenerate it only from a commit whose launches are the wanted ones, and say in the commit message which one:

    python tests/golden/gen_stage_trace.py [out.json]      (default tests/golden/stage_trace.json)

The file holds each distinct row once ("rows") and every case as a list of indices into them ("cases"). The stage is
reached through stage_apply alone, which knows the spelling with a separate FiLM function as well, so this script runs
unchanged on commits before the two were made one."""
import contextlib
import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for _p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "safe-dreamer_amd")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import torch  # noqa: E402

import conv_models as cm  # noqa: E402
from launch_trace import recorded  # noqa: E402

DEV = "cuda"
PATH = os.path.join(HERE, "stage_trace.json")
ANCHORS = {"a_32_48": (32, 48, 32), "a_48_64": (48, 64, 16)}  # test_gpu_conv_pooled_bwd.ANCHORS: ci, co, H = W
SWITCHES = ("pool_compact", "fused_pool", "conv6", "wgrad1_x3")
UPDATES = ("walker_r2", "walker_mm_r2")


def stage_apply(x, w, b, nw, nchw, pad_shift=None, film=None):
    from sdreamer import ops
    if film is None:
        return ops.ConvPoolNormFn.apply(x, w, b, nw, nchw, pad_shift)
    if "gamma" in inspect.signature(ops.ConvPoolNormFn.forward).parameters:
        return ops.ConvPoolNormFn.apply(x, w, b, nw, nchw, pad_shift, film[0], film[1])
    return ops.FilmConvPoolNormFn.apply(x, w, b, nw, film[0], film[1], nchw, pad_shift)


@contextlib.contextmanager
def switched(pool_compact=True, fused_pool=True, conv6=True, wgrad1_x3=True):
    from sdreamer import kernels as K, ops
    want = ((ops, "POOL_COMPACT", pool_compact), (ops, "FUSED_POOL", fused_pool), (K, "CONV6", conv6),
            (K, "WGRAD1_X3", wgrad1_x3))
    prev = [getattr(m, n) for m, n, _ in want]
    assert K.FAST_GEMM, "the trace is recorded with the split-bf16 kernels on"
    for m, n, v in want:
        setattr(m, n, v)
    try:
        yield
    finally:
        for (m, n, _), v in zip(want, prev):
            setattr(m, n, v)


def _trace(fn):
    from sdreamer import kernels as K
    K.clear_flip_cache()  # keyed by address: nothing an earlier case left may answer for this one's weights
    return recorded(fn, rows=True)[1]


def stage_case(c):
    from sdreamer import kernels as K
    x, w, b, nw, gamma, beta, dy = cm.stage_inputs(c)
    wd = w.permute(0, 2, 3, 1).contiguous().to(DEV).requires_grad_()
    bd, nwd = b.to(DEV).requires_grad_(), nw.to(DEV).requires_grad_()
    pad_shift = None
    if c.raw and c.dx:
        xd, pad_shift = x.to(DEV).requires_grad_(), 0.5
    elif c.raw:
        xd = K.pad_channels(x.to(DEV), c.cx, 0.5)
    else:
        xd = x.to(DEV).requires_grad_(c.dx)
    film = (gamma.to(DEV).requires_grad_(), beta.to(DEV).requires_grad_()) if c.ipc else None
    dyd = dy.to(DEV)
    with switched(wgrad1_x3=c.x3):
        return _trace(lambda: stage_apply(xd, wd, bd, nwd, c.nchw, pad_shift, film).backward(dyd))


def switch_case(anchor, film, dx, off):
    ci, co, hw = ANCHORS[anchor]
    g = lambda seed: torch.Generator().manual_seed(seed)  # noqa: E731
    x = torch.randn(2, hw, hw, ci, generator=g(20)).to(DEV).requires_grad_(dx)
    w = (torch.randn(co, 5, 5, ci, generator=g(21)) / (ci * 25) ** 0.5).to(DEV).requires_grad_()
    b = (0.1 * torch.randn(co, generator=g(22))).to(DEV).requires_grad_()
    nw = (1 + 0.1 * torch.randn(co, generator=g(23))).to(DEV).requires_grad_()
    fm = None
    if film:
        fm = ((1.5 + 0.2 * torch.randn(2, co, generator=g(24))).to(DEV).requires_grad_(),
              (0.1 * torch.randn(2, co, generator=g(25))).to(DEV).requires_grad_())
    dy = torch.randn(2, hw // 2, hw // 2, co, generator=g(26)).to(DEV)
    with switched(**{off: False}):
        return _trace(lambda: stage_apply(x, w, b, nw, False, None, fm).backward(dy))


def stage_cases():
    return {f"stage/{c.name}": stage_case(c) for c in cm.STAGE_CASES}


def switch_cases():
    return {f"switch/{a}-{'film' if film else 'plain'}-{'dx' if dx else 'nodx'}-{off}_off":
            switch_case(a, film, dx, off)
            for a in sorted(ANCHORS) for film in (False, True) for dx in (True, False) for off in SWITCHES}


def update_cases(name):
    """{update/<name>/update_batch, update/<name>/observation_grad}: each call traced after one call that is not"""
    from golden_io import batch, initial
    if name == "walker_r2":
        from test_gpu_dreamer import build_agent
        ag, z, spec, obs = build_agent(name)
        before, ctx = (lambda: None), (lambda: None)
    else:
        from test_gpu_multimodal_update import OBS as obs, _build, _force_text
        ag, z, spec, _, _ = _build(name)
        B, text = int(z["meta_B"]), int(z["u0_text"])
        before, ctx = (lambda: _force_text(ag, B, text)), (lambda: ag._posterior_text_ctx(B, text))
    ag.use_graphs = False
    data, init = batch(z, 0, obs, DEV), initial(z, 0, spec, DEV)
    out = {}
    with switched():
        for what in ("update_batch", "observation_grad"):
            for seed, keep in ((11, False), (12, True)):
                if what == "update_batch":
                    before()
                    fn = lambda: ag.update_batch(data, init, seed)  # noqa: E731
                else:
                    text_ctx = ctx()
                    fn = lambda: ag.observation_grad(  # noqa: E731
                        data, init, lambda ps, pd, pl: pl.square().mean() + pd.sum(), seed=seed, text_ctx=text_ctx)
                rows = _trace(fn) if keep else fn()
            out[f"update/{name}/{what}"] = rows
    return out


def pack(cases):
    """{case: rows} -> {"rows": the distinct rows, "cases": {case: indices into them}}"""
    index, packed = {}, {}
    for name, rows in cases.items():
        packed[name] = [index.setdefault(json.dumps(r), len(index)) for r in rows]
    return {"rows": [json.loads(k) for k in index], "cases": packed}


def unpack(doc):
    return {name: [doc["rows"][i] for i in idx] for name, idx in doc["cases"].items()}


def main(path):
    cases = {**stage_cases(), **switch_cases()}
    for name in UPDATES:
        cases.update(update_cases(name))
    doc = pack(cases)
    with open(path, "w") as f:
        f.write('{"rows": [\n' + ",\n".join(json.dumps(r) for r in doc["rows"]) + '\n],\n"cases": {\n' +
                ",\n".join(f"{json.dumps(k)}: {json.dumps(v, separators=(',', ':'))}"
                           for k, v in doc["cases"].items()) + "\n}}\n")
    print(f"{path}: {len(cases)} cases, {sum(map(len, cases.values()))} launches, {len(doc['rows'])} distinct rows")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else PATH)
