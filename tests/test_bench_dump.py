"""bench.py --dump-outputs, host side (CPU): the recorder around Buffer.update passes the write-back through unchanged
and keeps the latest posterior; dump_outputs writes one float32 .npy per metric and posterior array, cuts an array
above bench.DUMP_ARRAY_BYTES to the same fixed sample on every call, and stays under 64 MB in all."""
import os

import numpy as np
import torch

import bench


class _Buf:
    def __init__(self):
        self.calls = []

    def update(self, index, stoch, deter):
        self.calls.append((index, stoch, deter))
        return "written"


def test_last_posterior_passes_write_back_through():
    buf = _Buf()
    post = bench._LastPosterior(buf)
    index = [torch.zeros(2, 3), torch.ones(2, 3)]
    for i in range(2):
        s, d = torch.full((2, 3, 4, 4), float(i)), torch.full((2, 3, 8), float(i))
        assert buf.update(index, s, d) == "written"
        assert buf.calls[-1][0] is index and buf.calls[-1][1] is s and buf.calls[-1][2] is d
        assert post.stoch is s and post.deter is d


def test_dump_outputs_files_sample_and_size(tmp_path):
    g = torch.Generator().manual_seed(3)
    big = 3 * (bench.DUMP_ARRAY_BYTES // 12 + 7)  # an element count just above the per-array cap
    buf = _Buf()
    post = bench._LastPosterior(buf)
    buf.update(None, torch.rand(4, 5, 6, 7, generator=g), torch.rand(3, big // 3, generator=g))
    mets = {"loss/dyn": torch.tensor(1.5), "opt/lr": 1e-4, "ret/vec": torch.arange(3.0, dtype=torch.float64)}
    a, b = str(tmp_path / "a"), str(tmp_path / "b")
    bench.dump_outputs(a, mets, post)
    bench.dump_outputs(b, mets, post)
    assert sorted(os.listdir(a)) == ["loss.dyn.npy", "opt.lr.npy", "post_deter.npy", "post_stoch.npy", "ret.vec.npy"]
    got = {f: np.load(os.path.join(a, f)) for f in os.listdir(a)}
    assert all(v.dtype == np.float32 for v in got.values())
    assert got["loss.dyn.npy"].item() == 1.5 and got["opt.lr.npy"].item() == np.float32(1e-4)
    np.testing.assert_array_equal(got["ret.vec.npy"], [0.0, 1.0, 2.0])
    np.testing.assert_array_equal(got["post_stoch.npy"], post.stoch.numpy())  # below the cap: whole, in shape
    deter = got["post_deter.npy"]
    assert deter.nbytes == bench.DUMP_ARRAY_BYTES and deter.ndim == 1
    idx = np.sort(np.random.default_rng(0).integers(0, big, bench.DUMP_ARRAY_BYTES // 4))
    np.testing.assert_array_equal(deter, post.deter.numpy().reshape(-1)[idx])
    for f in got:  # the same arguments give the same files
        np.testing.assert_array_equal(got[f], np.load(os.path.join(b, f)))
    assert 2 * bench.DUMP_ARRAY_BYTES + (1 << 20) <= 64 << 20  # two capped arrays + the metrics
