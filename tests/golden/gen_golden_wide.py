"""Golden vectors of the reference's own ConvEncoder (world_model/networks.py:192-234) at model.depth=77, the width
of its parameter-matched wider-CNN baseline: tests/golden/encoder_wide_h3.npz.

Runs where the reference is importable only (see refimport.py); the fixture it writes is data. Parameters, the 2
frames and the probe of the loss come from the seeded formulas in tests/wide_golden_io.py, shared with the tests: no
weights are stored. The fixture holds the 2 x 4928 outputs and, under the probe loss sum(out * probe), every
parameter gradient's L2 norm and 32 sampled elements.

    python tests/golden/gen_golden_wide.py
"""
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "safe-dreamer_amd"), os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import wide_golden_io as wg  # noqa: E402
from refimport import import_reference  # noqa: E402


def main():
    torch.set_num_threads(8)
    mods, _ = import_reference()
    N = mods["world_model.networks"]
    cfg = types.SimpleNamespace(act="SiLU", norm=True, kernel_size=wg.KS, depth=wg.DEPTH, mults=list(wg.MULTS))
    enc = N.ConvEncoder(cfg, (64, 64, 3))
    assert enc.out_dim == 4928 and enc.depths == wg.WIDTHS
    sd = enc.state_dict()
    want = {k[len(wg.PREFIX):]: v for k, v in wg.params().items()}
    assert list(sd) == list(want), (list(sd), list(want))
    assert all(tuple(sd[k].shape) == want[k].shape for k in sd)
    enc.load_state_dict({k: torch.from_numpy(v) for k, v in want.items()})
    out = enc(torch.from_numpy(wg.frames()))  # (2, 1, 4928)
    out = out.reshape(wg.FRAMES, -1)
    loss = (out * torch.from_numpy(wg.probe())).sum()
    loss.backward()
    grads = {wg.PREFIX + k: p.grad.numpy() for k, p in enc.named_parameters()}
    arrs = wg.summarise(out.detach().numpy(), grads)
    arrs["loss"] = np.asarray(float(loss.detach()))
    np.savez_compressed(wg.FIXTURE, **arrs)
    print(f"{wg.FIXTURE}: {len(arrs)} arrays, {os.path.getsize(wg.FIXTURE)} bytes, loss {float(loss):.6g}")


if __name__ == "__main__":
    main()
