"""Per-kernel A/B of two trees from four kernel-trace runs of bench.py, alternated (this tree, parent, this tree,
parent): markdown rows of ms per update inside bench.py's timed window, from the JSON tools/kernel_table.py writes per
run, summed over every launch grid of a kernel name.

Usage: python tools/kernel_ab_table.py <this 1.json> <parent 1.json> <this 2.json> <parent 2.json> [name filter ...]
A filter written changed=<substring> also marks the kernels it matches as `changed` in the code column (their
instruction text differs from the parent's, as compared by hand with hipcc -S); every other kernel is `same`.
grid: rows per (kernel, launch grid) instead of per kernel name (one template instance at several stages).
alias=<this tree's substring>=><parent's substring>: a kernel this tree launches under another name (a template flag
added or turned) is listed in the parent's row, named `parent's name (this tree: its name)`.

flag: GAINED = both runs of this tree below both of the parent and the difference of the means above the parent's own
run-to-run difference; GREW = the same with the signs turned (the rule of profiles/gemm_core_refactor_kernel_table.md).
Kernels matching a name filter are listed first; without filters the order is the parent's time."""
import collections
import json
import sys


def load(path, by_grid=False, alias=(), shown=None):
    per, n = collections.defaultdict(float), collections.defaultdict(float)
    for r in json.load(open(path))["rows"]:
        k = r["kernel"]
        was = k
        for new, old in alias:
            if new in k:
                k = k.replace(new, old)
        if by_grid:
            k += " @ " + "x".join(map(str, r["grid"]))
        if shown is not None and was != r["kernel"].replace(was, k.split(" @ ")[0]):
            shown[k] = was
        per[k] += r["ms_per_update"]
        n[k] += r["launches_per_update"]
    return per, n


def main(t1, p1, t2, p2, *filters):
    by_grid = "grid" in filters
    alias = [tuple(f[len("alias="):].split("=>")) for f in filters if f.startswith("alias=")]
    filters = [f for f in filters if f != "grid" and not f.startswith("alias=")]
    shown = {}
    (a1, n1), (a2, _) = load(t1, by_grid, alias, shown), load(t2, by_grid, alias, shown)
    (b1, _), (b2, _) = load(p1, by_grid), load(p2, by_grid)
    names = sorted(set(a1) | set(b1) | set(a2) | set(b2), key=lambda k: -(b1.get(k, 0.0) + b2.get(k, 0.0)))
    changed = [f[len("changed="):] for f in filters if f.startswith("changed=")]
    filters = [f[len("changed="):] if f.startswith("changed=") else f for f in filters]
    first = [k for k in names if any(f in k for f in filters)]
    print("| kernel | code | launches / update | parent | parent again | this tree | this tree again | this - parent (means) "
          "| parent run-to-run | flag |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    tot = [0.0] * 4
    for k in first + [k for k in names if k not in first]:
        v = [b1.get(k, 0.0), b2.get(k, 0.0), a1.get(k, 0.0), a2.get(k, 0.0)]
        tot = [s + x for s, x in zip(tot, v)]
        d, rr = (v[2] + v[3]) / 2 - (v[0] + v[1]) / 2, abs(v[0] - v[1])
        flag = ""
        if max(v[2:]) < min(v[:2]) and -d > rr:
            flag = "GAINED"
        elif min(v[2:]) > max(v[:2]) and d > rr:
            flag = "GREW"
        code = "changed" if any(c in k for c in changed) else "same"
        name = f"{k} (this tree: {shown[k]})" if k in shown else k
        print(f"| {name} | {code} | {n1.get(k, 0.0):.1f} | {v[0]:.4f} | {v[1]:.4f} | {v[2]:.4f} | {v[3]:.4f} | {d:+.4f} | {rr:.4f} "
              f"| {flag} |")
    d = (tot[2] + tot[3]) / 2 - (tot[0] + tot[1]) / 2
    print(f"| **sum** | | | {tot[0]:.4f} | {tot[1]:.4f} | {tot[2]:.4f} | {tot[3]:.4f} | {d:+.4f} | {abs(tot[0] - tot[1]):.4f} | |")


if __name__ == "__main__":
    main(*sys.argv[1:])
