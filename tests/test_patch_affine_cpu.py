"""CPU side of the affine / photometric EoT: the host functions of sdreamer.attack (transform_rows, eot_transforms, the
configuration keys, the generators), and the case table of tests/patch_affine_ref.py judged by its own bounds (the
float32 restatement passes them, every planted fault fails one)."""
import math

import pytest
import torch

import patch_affine_ref as par


def test_transform_rows_identity_centre_and_hand_computed_points():
    from sdreamer.attack import transform_rows
    ph, pw = 5, 7
    # s = 1, theta = 0: the identity row of the offset
    r = transform_rows([[3, -4], [0, 0]], [[1.0, 0.0, 1.0, 0.0]] * 2, (ph, pw))
    assert r.dtype == torch.float32 and r.shape == (2, 8)
    assert torch.equal(r, torch.tensor([[1, 0, -3, 0, 1, 4, 1, 0], [1, 0, 0, 0, 1, 0, 1, 0]], dtype=torch.float32))
    assert not bool(torch.signbit(r[:, [1, 3]]).any())  # no negative zeros
    # any scale and angle: the patch's centre maps to itself
    g = torch.Generator().manual_seed(0)
    par4 = torch.rand(16, 4, generator=g, dtype=torch.float64) + 0.5
    offs = torch.randint(-5, 20, (16, 2), generator=g)
    r = transform_rows(offs, par4, (ph, pw)).double()
    cy, cx = offs[:, 0] + (ph - 1) / 2, offs[:, 1] + (pw - 1) / 2
    u = r[:, 0] * cy + r[:, 1] * cx + r[:, 2]
    v = r[:, 3] * cy + r[:, 4] * cx + r[:, 5]
    assert float((u - (ph - 1) / 2).abs().max()) < 1e-5 and float((v - (pw - 1) / 2).abs().max()) < 1e-5
    assert torch.equal(r[:, 6:].float(), par4[:, 2:].float())
    # 90 degrees about the centre (4, 6) of a patch at (2, 3): one pixel to the right of the centre shows the patch
    # element one row below the patch's centre ([u; v] = R(-theta) d = [[0, 1], [-1, 0]] d), one pixel below it the
    # element one column to the left
    r = transform_rows([[2, 3]], [[1.0, math.pi / 2, 1.0, 0.0]], (ph, pw)).double()[0]
    at = lambda y, x: (float(r[0] * y + r[1] * x + r[2]), float(r[3] * y + r[4] * x + r[5]))  # noqa: E731
    assert at(4, 7) == pytest.approx((3.0, 3.0), abs=1e-6)
    assert at(5, 6) == pytest.approx((2.0, 2.0), abs=1e-6)
    # scale 2 about the same centre: two pixels in the image are one patch element
    r = transform_rows([[2, 3]], [[2.0, 0.0, 1.0, 0.0]], (ph, pw)).double()[0]
    assert at(4, 6) == pytest.approx((2.0, 3.0), abs=1e-6)
    assert at(6, 6) == pytest.approx((3.0, 3.0), abs=1e-6)
    assert at(4, 3) == pytest.approx((2.0, 1.5), abs=1e-6)
    assert at(0, 0) == pytest.approx((0.0, 0.0), abs=1e-6)
    for s in (0.0, -1.0):
        with pytest.raises(ValueError, match="scale"):
            transform_rows([[0, 0]], [[s, 0.0, 1.0, 0.0]], (ph, pw))
    with pytest.raises(ValueError, match="finite"):
        transform_rows([[0, 0]], [[1.0, float("nan"), 1.0, 0.0]], (ph, pw))
    from sdreamer.attack import check_rows
    with pytest.raises(ValueError, match="singular"):
        check_rows(torch.tensor([[1.0, 2.0, 0.0, 2.0, 4.0, 0.0, 1.0, 0.0]]))


def test_eot_transforms_shapes_ranges_and_seed():
    from sdreamer.attack import eot_transforms
    kw = dict(scale=(0.75, 1.25), rotation_deg=20.0, contrast=0.3, brightness=0.1)
    a = eot_transforms(6, 3, torch.Generator().manual_seed(5), **kw)
    b = eot_transforms(6, 3, torch.Generator().manual_seed(5), **kw)
    assert a.shape == (24, 4) and a.dtype == torch.float64 and torch.equal(a, b)
    assert torch.equal(a[:6], torch.tensor([[1.0, 0.0, 1.0, 0.0]] * 6, dtype=torch.float64))
    s, th, gain, bias = a[6:].unbind(1)
    assert 0.75 <= float(s.min()) and float(s.max()) <= 1.25 and float(s.max() - s.min()) > 0.1
    lim = 20.0 * math.pi / 180
    assert float(th.abs().max()) <= lim and float(th.min()) < 0 < float(th.max())
    assert 0.7 <= float(gain.min()) and float(gain.max()) <= 1.3 and float(gain.min()) < 1 < float(gain.max())
    assert float(bias.abs().max()) <= 0.1 and float(bias.min()) < 0 < float(bias.max())
    # one rand((n * copies, 4)) call: the generator's state afterwards says so
    g1, g2 = torch.Generator().manual_seed(5), torch.Generator().manual_seed(5)
    eot_transforms(6, 3, g1, **kw)
    torch.rand((18, 4), generator=g2, dtype=torch.float64)
    assert torch.equal(g1.get_state(), g2.get_state())
    # ranges off: every row the identity; no copies: no draw
    off = eot_transforms(4, 2, torch.Generator().manual_seed(1))
    assert torch.equal(off, torch.tensor([[1.0, 0.0, 1.0, 0.0]] * 12, dtype=torch.float64))
    g3 = torch.Generator().manual_seed(5)
    eot_transforms(4, 0, g3, **kw)
    assert torch.equal(g3.get_state(), torch.Generator().manual_seed(5).get_state())


def test_offsets_are_unchanged_by_the_transform_draws():
    """AdversarialPatch.generator's sequence (offsets, saliency noise) is what eot_offsets alone draws from the same
    seed, whether or not the transform ranges are on: they draw from transform_generator."""
    from sdreamer.attack import TRANSFORM_SEED_OFFSET, AdversarialPatch, eot_offsets, eot_transforms, transform_rows
    kw = dict(image_hw=(12, 20), patch_hw=(5, 7), eot_translations=2, max_jitter=3, seed=11, device="cpu")
    on = AdversarialPatch(**kw, eot_scale=(0.8, 1.2), eot_rotation=15.0, eot_contrast=0.2, eot_brightness=0.1)
    plain = AdversarialPatch(**kw)
    ref = torch.Generator().manual_seed(11)
    tgen = torch.Generator().manual_seed(11 + TRANSFORM_SEED_OFFSET)
    assert plain.transforms(4) is None and on.transforms(4, jitter=False) is None
    for _ in range(3):
        want = eot_offsets(on.offset, 4, 2, ref, 3)
        a = on.offsets(4)
        rows = on.transforms(4)
        assert torch.equal(a, want) and torch.equal(plain.offsets(4), want)
        assert torch.equal(on.generator.get_state(), ref.get_state())
        assert torch.equal(rows, transform_rows(want, eot_transforms(4, 2, tgen, (0.8, 1.2), 15.0, 0.2, 0.1), (5, 7)))
        assert rows.shape == (12, 8) and torch.equal(rows[:4], transform_rows(want[:4], [[1.0, 0.0, 1.0, 0.0]] * 4, (5, 7)))
    # without an offsets() call of that size the rows sit at the base offset
    rows = on.transforms(2)
    assert torch.equal(rows[:2, [2, 5]], -torch.tensor([on.offset] * 2, dtype=torch.float32))


def test_config_keys_default_off_and_need_copies():
    from sdreamer.attack import AdversarialPatch, eot_ranges, load_attack_config
    cfg = load_attack_config()
    assert list(cfg.eot_scale) == [1.0, 1.0] and cfg.eot_rotation == 0.0 and cfg.eot_contrast == 0.0
    assert cfg.eot_brightness == 0.0
    assert eot_ranges(cfg) == ((1.0, 1.0), 0.0, 0.0, 0.0)
    cfg = load_attack_config(["eot_translations=2", "max_jitter=0", "eot_scale=[0.8,1.25]", "eot_rotation=20",
                              "eot_contrast=0.2", "eot_brightness=0.1"])
    assert eot_ranges(cfg) == ((0.8, 1.25), 20.0, 0.2, 0.1) and cfg.max_jitter == 0
    for key, val in (("eot_scale", "[0.9,1.1]"), ("eot_rotation", "10"), ("eot_contrast", "0.1"),
                     ("eot_brightness", "0.05")):
        with pytest.raises(ValueError, match=key):
            load_attack_config([f"{key}={val}"])
        load_attack_config([f"{key}={val}", "eot_translations=1"])
    with pytest.raises(ValueError, match="eot_rotation"):
        AdversarialPatch(device="cpu", eot_rotation=5.0)
    with pytest.raises(ValueError, match="eot_scale"):
        load_attack_config(["eot_scale=[0.0,1.0]", "eot_translations=1"])


@pytest.fixture(scope="module")
def table():
    inp = par.inputs()
    cases = par.case_table()
    ref = {}
    for name, tf in cases.items():
        for kind in ("u8", "f32"):
            img = inp[kind].double() / 255 if kind == "u8" else inp[kind].double()
            ref[name, kind] = (par.composite(img, inp["patch"], tf).detach(),
                               par.gradient(img, inp["patch"], tf, inp["dimg"]))
    return inp, cases, ref


def _fractions(inp, tf, ref, kind, dtype, fault=None):
    """(the largest forward error, the largest gradient error) of the restatement, as fractions of the bounds"""
    img = inp[kind].double() / 255 if kind == "u8" else inp[kind].double()
    img = img.to(dtype)  # the f32 restatement starts from the f32 image, as the kernel does
    out = par.composite(img, inp["patch"], tf, dtype, fault).detach().double()
    grad = par.gradient(img, inp["patch"], tf, inp["dimg"], dtype, fault).double()
    return (float(((out - ref[0]).abs() / par.forward_bound(tf)).max()),
            float(((grad - ref[1]).abs() / par.gradient_bound(tf, inp["dimg"]).clamp_min(1e-300)).max()))


def test_case_table_covers_what_it_names(table):
    inp, cases, ref = table
    assert set(cases) == {"identity", "subpixel", "rot90", "rotation", "scale", "scale2_half_off", "off_image",
                          "photometric"}
    for name, tf in cases.items():
        assert tf.shape == (par.NB, 8) and tf.dtype == torch.float32
        assert par.margin(inp["patch"], tf) >= par.MARGIN, name
    assert par.NB > par.CHUNK and par.PH != par.PW
    w = {name: par.hat_weights(tf)[0] for name, tf in cases.items()}
    alpha = {name: v.sum(dim=(3, 4)) for name, v in w.items()}
    assert float(alpha["off_image"].max()) == 0.0  # wholly off the image
    assert torch.equal(ref["off_image", "u8"][0], inp["u8"].double() / 255)
    assert not bool(ref["off_image", "f32"][1].any())
    ident = cases["identity"]
    assert torch.equal(ident[:, [0, 1, 3, 4, 6, 7]], torch.tensor([[1.0, 0, 0, 1, 1, 0]] * par.NB))
    assert torch.equal(ident[:, [2, 5]], ident[:, [2, 5]].round())
    covered = alpha["identity"].sum(dim=(1, 2))
    assert float(covered.max()) == par.PH * par.PW and 0 < float(covered[0]) < par.PH * par.PW  # whole and clipped
    frac = cases["subpixel"][:, [2, 5]]
    assert bool(((frac - frac.round()).abs() > 1e-3).any())
    assert torch.equal(cases["rot90"][:, [0, 1, 3, 4]], torch.tensor([[0.0, 1, -1, 0]] * par.NB))
    a2 = alpha["scale2_half_off"].sum(dim=(1, 2))  # a window of about 10 x 14 pixels, at most two thirds of it lands
    assert float(a2.min()) > 0 and float(a2.max()) < 0.67 * 4 * par.PH * par.PW
    # the photometric case clamps some elements at each end, and not all
    _, lin = par.photometric(inp["patch"], cases["photometric"], torch.float64)
    assert bool((lin > 1).any()) and bool((lin < 0).any()) and bool(((lin > 0) & (lin < 1)).any())
    # the tap formulation is the hat formulation: out = sum_ij W P + (1 - sum_ij W) in, in float64
    for name in ("rotation", "scale2_half_off", "photometric"):
        P, _ = par.photometric(inp["patch"], cases[name], torch.float64)
        want = torch.einsum("nyxij,nijc->nyxc", w[name], P) + (1 - alpha[name]).unsqueeze(-1) * inp["f32"].double()
        assert float((want - ref[name, "f32"][0]).abs().max()) < 1e-12, name


def test_f32_restatement_passes_both_bounds_in_every_case(table):
    inp, cases, ref = table
    worst = [0.0, 0.0]
    for name, tf in cases.items():
        for kind in ("u8", "f32"):
            f, g = _fractions(inp, tf, ref[name, kind], kind, torch.float32)
            print(f"{name:16s} {kind:3s}: forward {f:.3f}, gradient {g:.3f} of the bound")
            assert f <= 1.0 and g <= 1.0, (name, kind, f, g)
            worst = [max(worst[0], f), max(worst[1], g)]
    print(f"f32 restatement: at most {worst[0]:.3f} of the forward bound, {worst[1]:.3f} of the gradient bound")


@pytest.mark.parametrize("fault", par.FAULTS)
def test_every_planted_fault_fails_a_case(table, fault):
    inp, cases, ref = table
    worst = max(max(_fractions(inp, tf, ref[name, "f32"], "f32", torch.float32, fault)) for name, tf in cases.items())
    print(f"{fault}: {worst:.3g} of a bound")
    assert worst > 1.0
