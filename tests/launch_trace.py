"""Every C-ABI launch (nat.call / nat.call_shaped) made while a function runs, seen through nat.PROBES.

names: the entry names in order. rows: one [name, arg, ...] per launch, keeping what does not depend on where the
allocator put a buffer: a float or an int below 2^31 verbatim (shapes, strides, flags, seeds, scales; 0 is also how
kernels.p spells a null pointer and the default stream), anything else (device pointers, struct addresses, a side
stream) as None when it is null and "*" when it is not. A call_shaped that its entry refuses is recorded as well: it is
part of the sequence the Python layer issues."""
import torch


class Launches:
    """matches no launch (so times none); records each one it is asked about"""

    def __init__(self):
        self.names, self.rows = [], []

    @staticmethod
    def _arg(a):
        if isinstance(a, float) or (isinstance(a, int) and a < 2 ** 31):
            return a
        return None if not a else "*"

    def match(self, name, args):
        self.names.append(name)
        self.rows.append([name] + [self._arg(a) for a in args])
        return False


def recorded(fn, rows=False):
    """-> (fn(), the launches' names, or their rows)"""
    from sdreamer import _native as nat
    rec = Launches()
    nat.PROBES.append(rec)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        nat.PROBES.remove(rec)
    return out, (rec.rows if rows else rec.names)
