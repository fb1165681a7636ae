"""CPU side of the image-gradient / adversarial-patch feature: the ABI entries, the attack config, the placement
arithmetic, and the oracle against the reference's image-gradient fixture (tests/golden/walker_r2_imgrad.npz)."""
import os
import re

import numpy as np
import pytest
import torch

import imgrad_ref as ir
from golden_io import load_case

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_ENTRIES = ("sd_conv2d_dgrad_pool", "sd_conv2d_dgrad_pool_ok", "sd_patch_apply", "sd_patch_grad", "sd_patch_step")


def test_new_entries_declared_and_exported():
    from sdreamer import _native as nat
    text = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "sdhip.h")).read(), flags=re.S)
    declared = sorted(set(re.findall(r"\bint\s+(sd_\w+)\s*\(", text)))
    assert sorted(nat.exported_symbols()) == declared
    for n in NEW_ENTRIES:
        assert n in declared and hasattr(nat.lib, n), n
    assert nat.ABI_VERSION == 1
    assert "sd_conv2d_dgrad_pool_film" not in declared  # one kernel serves both stage Functions


def test_attack_config_defaults_and_overrides():
    from sdreamer.attack import load_attack_config
    cfg = load_attack_config()
    assert list(cfg.patch_hw) == [16, 16] and cfg.placement == "bottom_center" and cfg.eps is None
    assert cfg.w_tv == 0.01 and cfg.eot_translations == 0 and cfg.steps == 5000 and cfg.lr == 0.05
    assert cfg.w_return == 0.0 and cfg.w_kl == 1.0 and cfg.w_action == 0.0
    assert cfg.x0 == 0 and cfg.y0 == 0
    cfg = load_attack_config(["steps=7", "placement=fixed", "x0=3", "y0=-2", "eps=0.1", "patch_hw=[8,12]"])
    assert (cfg.steps, cfg.placement, cfg.x0, cfg.y0, cfg.eps, list(cfg.patch_hw)) == (7, "fixed", 3, -2, 0.1, [8, 12])


def test_return_term_is_refused():
    from sdreamer.attack import PosteriorAttackLoss
    PosteriorAttackLoss(w_kl=1.0, w_action=1.0, w_tv=0.01)
    with pytest.raises(NotImplementedError, match="imagination"):
        PosteriorAttackLoss(w_kl=1.0, w_action=0.0, w_tv=0.01, w_return=1.0)


def test_placement_arithmetic():
    from sdreamer.attack import clipped_window, eot_offsets, placement_offset, saliency_offset
    hw, p = (64, 64), (16, 16)
    assert placement_offset("bottom_center", hw, p) == (48, 24)
    assert placement_offset("top_center", hw, p) == (0, 24)
    assert placement_offset("center", hw, p) == (24, 24)
    assert placement_offset("fixed", hw, p, x0=5, y0=-3) == (-3, 5)
    assert placement_offset("bottom_center", (64, 48), (10, 7)) == (54, 20)
    with pytest.raises(ValueError):
        placement_offset("saliency", hw, p)
    with pytest.raises(ValueError):
        placement_offset("left", hw, p)
    # clipping: inside, over each border, over a corner, entirely outside
    assert clipped_window((24, 24), hw, p) == ((24, 40, 24, 40), (0, 0))
    assert clipped_window((-5, 10), hw, p) == ((0, 11, 10, 26), (5, 0))
    assert clipped_window((20, -7), hw, p) == ((20, 36, 0, 9), (0, 7))
    assert clipped_window((60, 55), hw, p) == ((60, 64, 55, 64), (0, 0))
    (y0, y1, x0, x1), _ = clipped_window((100, 100), hw, p)
    assert y1 <= y0 and x1 <= x0
    (y0, y1, x0, x1), _ = clipped_window((-16, 0), hw, p)
    assert y1 <= y0
    # saliency: the window with the largest sum, brute force on a random map; the first one on a tie
    sal = torch.rand(20, 17, generator=torch.Generator().manual_seed(0))
    best = max(((float(sal[y:y + 4, x:x + 5].sum()), -y, -x) for y in range(17) for x in range(13)))
    assert saliency_offset(sal, (4, 5)) == (-best[1], -best[2])
    assert saliency_offset(torch.zeros(8, 8), (3, 3)) == (0, 0)
    spot = torch.zeros(64, 64)
    spot[63, 63] = 1.0
    assert saliency_offset(spot, p) == (48, 48)
    # EoT offsets: the first copy sits at the base, the others within the jitter, the same for the same seed
    a = eot_offsets((48, 24), 6, 2, torch.Generator().manual_seed(3), 4)
    b = eot_offsets((48, 24), 6, 2, torch.Generator().manual_seed(3), 4)
    assert a.shape == (18, 2) and a.dtype == torch.int32 and torch.equal(a, b)
    assert torch.equal(a[:6], torch.tensor([[48, 24]] * 6, dtype=torch.int32))
    d = a[6:] - torch.tensor([48, 24], dtype=torch.int32)
    assert int(d.abs().max()) <= 4 and int(d.abs().max()) > 0


def test_oracle_matches_reference_image_gradient():
    """The oracle's encode + observe under autograd against the reference's own image gradient of the probe loss
    (fixture): posterior indices exact; in f32 the per-frame norms and the 4,096 sampled elements equal the
    reference's to rounding (measured: identical), in float64 they reproduce the fixture's float64 values. The f32 to
    float64 distance (measured: norms 3.6e-7 relative, elements 0.0077 of the gradient test's element bound 2e-3 |g| +
    1e-4 max |g|) is far below half of the GPU test's bounds (norms 2e-4, elements 1.0), so the GPU test compares
    against the reference's f32 values on those bounds unchanged."""
    z = ir.load_fixture()
    _, cfg, spec, params, obs = load_case("walker_r2")
    data, init = ir.fixture_inputs(z, obs, spec)
    assert float(z["meta_min_gap"]) >= 2e-4
    ref32, ref64 = (z["g_norm"], z["g_s"].astype(np.float64)), (z["g64_norm"], z["g64_s"])
    g, idx, loss = ir.oracle_image_grad(spec, params, data, init, int(z["seed"]), z["R"], torch.float32)
    assert g.shape == (2, 6, 64, 64, 3) and np.array_equal(idx, z["post_idx"])
    dn, de = ir.distance(*ir.sampled(g), *ref32)
    print(f"oracle f32 vs reference f32: norm {dn:.2e}, element {de:.2e} of the bound")
    assert dn <= 1e-5 and de <= 1e-2
    assert abs(loss - float(z["loss"])) <= 1e-5 * abs(float(z["loss"]))
    g, idx, loss = ir.oracle_image_grad(spec, params, data, init, int(z["seed"]), z["R"], torch.float64)
    assert np.array_equal(idx, z["post_idx"])
    dn, de = ir.distance(*ir.sampled(g), *ref64)
    print(f"oracle float64 vs fixture float64: norm {dn:.2e}, element {de:.2e} of the bound")
    assert dn <= 1e-9 and de <= 1e-6
    dn, de = ir.distance(*ref32, *ref64)
    print(f"reference f32 vs float64: norm {dn:.2e}, element {de:.2e} of the bound")
    assert dn <= 1e-4 and de <= 0.5  # half of the GPU test's bounds: they stay as they are
