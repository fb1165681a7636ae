"""Acting latency: Dreamer.policy_graph(fused=False) (act, per-op after the encoder) against policy_graph(fused=True)
(policy_step: one sd_policy_step after the encoder) on the default workload's agent (walker r2dreamer, bench.py's
config), in one process.

  python tools/policy_latency.py [--batches 1,16,64] [--replays 5000] [--warmup 200] [--rounds 3]
      per B: the two graphs alternated `rounds` times, each window `replays` graph replays between two device events
      after `warmup` replays -> us per step of each path, the spread (max - min) of its windows, the weight bytes one
      step must read (from the shapes) and the share of the HBM peak they imply at the measured time.
  python tools/policy_latency.py --eager PATH --calls 10 [--batch 16]
      `calls` eager calls of one path (PATH = act | policy_step) after one warm-up call, for a kernel trace of its own
      (rocprofv3 --kernel-trace --stats -- python tools/policy_latency.py --eager policy_step): the kernel count per
      call is the trace's calls / `calls`, minus the encoder's. The calls sit between two sd_trace_mark dispatches.
  python tools/policy_latency.py --table TRACE_DIR --calls 10
      the kernels between the two marks of such a trace: launches per call and us per launch, as markdown.

The replays time the graph alone (device events around the loop; the static-input copies policy() makes per call are
outside, as both paths make the same ones). One JSON line at the end."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "safe-dreamer_amd"))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import bench  # noqa: E402

HBM_PEAK = 8.0e12  # bytes / s, MI355X


def build(B):
    from sdreamer.config import load_config
    from sdreamer.dreamer import Dreamer
    cfg = load_config("dmc/cnn", ["device=cuda:0", "model.compile=False"])
    torch.manual_seed(0)
    ag = Dreamer(cfg.model, bench._Spaces({"image": bench._Sp((64, 64, 3))}), bench._Sp((6,)))
    obs = {"image": torch.randint(0, 256, (B, 64, 64, 3), dtype=torch.uint8, device="cuda"),
           "is_first": torch.zeros(B, dtype=torch.bool, device="cuda")}
    return ag, obs


def weight_bytes(ag):
    """f32 bytes of every parameter one acting step reads after the encoder, from the shapes"""
    r, a = ag.rssm, ag.actor
    dn = r._deter_net
    groups = {
        "_dyn_in0/1/2": [p for m in (dn._dyn_in0, dn._dyn_in1, dn._dyn_in2) for p in m.parameters()],
        "_dyn_hid": list(dn._dyn_hid.parameters()),
        "_dyn_gru": list(dn._dyn_gru.parameters()),
        "obs_net": list(r._obs_net.parameters()),
        "actor": list(a.parameters()),
    }
    out = {k: 4 * sum(p.numel() for p in v) for k, v in groups.items()}
    out["total"] = sum(out.values())
    return out


def window(g, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / n  # us per replay


def latency(args):
    rows = []
    for B in [int(b) for b in args.batches.split(",")]:
        ag, obs = build(B)
        wb = weight_bytes(ag)
        state = ag.get_initial_state(B)
        paths = {"per_op": ag.policy_graph(B, obs), "fused": ag.policy_graph(B, obs, fused=True)}
        for p in paths.values():  # one call through policy(): the static inputs hold a real observation and state
            p(obs, state)
        times = {k: [] for k in paths}
        for _ in range(args.rounds):
            for k, p in paths.items():
                for _ in range(args.warmup):
                    p.graph.replay()
                times[k].append(window(p.graph, args.replays))
        row = dict(B=B, fused_admitted=bool(ag._fused_policy_ok(B)), weight_bytes=wb)
        for k, t in times.items():
            mean = sum(t) / len(t)
            row[k] = dict(us=round(mean, 2), spread_us=round(max(t) - min(t), 2), windows=[round(x, 2) for x in t],
                          hbm_share=round(wb["total"] / (mean * 1e-6) / HBM_PEAK, 4))
        row["fused_faster_by_us"] = round(row["per_op"]["us"] - row["fused"]["us"], 2)
        rows.append(row)
        print(f"B={B}: per-op graph {row['per_op']['us']} us (spread {row['per_op']['spread_us']}), fused graph "
              f"{row['fused']['us']} us (spread {row['fused']['spread_us']}); weights {wb['total'] / 1e6:.2f} MB",
              flush=True)
        del ag, paths
    print(json.dumps(dict(tool="policy_latency", replays=args.replays, warmup=args.warmup, rounds=args.rounds,
                          rows=rows)))


def eager(args):
    from launch_trace import recorded
    B = args.batch
    ag, obs = build(B)
    fn = getattr(ag, args.eager)
    state = ag.get_initial_state(B)
    fn(obs, state, seed=1, step=0)
    torch.cuda.synchronize()
    _, names = recorded(lambda: fn(obs, state, seed=1, step=0))
    with torch.no_grad():
        _, enc = recorded(lambda: ag.encoder({"image": ag.preprocess(dict(obs))["image"].unsqueeze(1)}))
    bench.trace_mark(1)  # the kernel trace's window (--table): the timed calls only
    for k in range(args.calls):
        fn(obs, state, seed=2 + k, step=0)
    bench.trace_mark(2)
    torch.cuda.synchronize()
    print(json.dumps(dict(tool="policy_latency", eager=args.eager, B=B, calls=args.calls,
                          abi_launches_per_call=len(names), abi_launches_after_encoder=len(names) - len(enc),
                          names=names)))


def table(args):
    """markdown table of the kernels between the two marks of an --eager run's trace directory"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_table
    tr, span = kernel_table.window(args.table)
    n = sum(len(v) for v in tr.values())
    print(f"{n} kernels in the window, {n / args.calls:.1f} per call; {sum(sum(v) for v in tr.values()) / args.calls / 1e3:.1f} "
          f"us of kernel time per call, {span / args.calls / 1e3:.1f} us wall per call\n")
    print("| kernel | grid | launches / call | us / launch |\n|---|---|---|---|")
    for (k, gx, gy, gz), d in sorted(tr.items(), key=lambda kv: -sum(kv[1])):
        print(f"| {k} | {gx}x{gy}x{gz} | {len(d) / args.calls:g} | {sum(d) / len(d) / 1e3:.2f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", default="1,16,64")
    ap.add_argument("--replays", type=int, default=5000)
    ap.add_argument("--warmup", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--eager", choices=["act", "policy_step"])
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--table", help="trace directory of an --eager run under rocprofv3 --kernel-trace")
    args = ap.parse_args()
    if args.table:
        table(args)
    elif args.eager:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        eager(args)
    else:
        latency(args)


if __name__ == "__main__":
    main()
