"""ops._stage_route, the one place a conv encoder stage's backward route is chosen, against the three expressions it
replaced (ConvPoolNormFn.backward's `first`, ops._pooled_dx and ops._pooled_x3 as they stood), written out below: the
four kernels.py queries and ops.POOL_COMPACT forced to every combination of answers, the input gradient wanted or not,
the conv input channel-padded (Cx != Ci) or not: 2^7 = 128 rows. Shapes only: no GPU."""
import itertools

import torch

QUERIES = ("conv2d_wgrad_pool_slabs", "conv2d_dgrad_pool_takes", "conv2d_wgrad_pooled_slabs",
           "conv2d_dgrad_pooled_takes")


def _before(need_dx, padded, compact, pool_slabs, pool_takes, pooled_slabs, pooled_takes):
    pooled_dx = need_dx and padded and compact and pool_slabs > 0 and pool_takes
    first = pooled_dx or (not need_dx and compact and pool_slabs > 0)
    if not compact or pooled_slabs <= 0:
        pooled_x3 = False
    else:
        pooled_x3 = not need_dx or (not padded and pooled_takes)
    x3 = not first and pooled_x3
    return "first" if first else "x3" if x3 else "full"


def test_stage_route_is_the_three_expressions_it_replaced(monkeypatch):
    from sdreamer import kernels as K, ops
    w = torch.empty(32, 5, 5, 3)
    rows = list(itertools.product((False, True), repeat=7))
    seen = set()
    for need_dx, padded, compact, *answers in rows:
        monkeypatch.setattr(ops, "POOL_COMPACT", compact)
        # the slab counts are ints (0: the plan refuses the shape), the takes are bools
        vals = [2 * a if name.endswith("slabs") else a for name, a in zip(QUERIES, answers)]
        for name, v in zip(QUERIES, vals):
            monkeypatch.setattr(K, name, lambda *args, _v=v, **kw: _v)
        x = torch.empty(2, 16, 64, 4 if padded else 3)
        got = ops._stage_route(need_dx, x, w)
        assert got == _before(need_dx, padded, compact, *vals), (need_dx, padded, compact, vals)
        seen.add(got)
    assert len(rows) == 128 and seen == {"first", "x3", "full"}
