"""The resampling patch kernels (csrc/attack.hip: sd_patch_apply_affine, sd_patch_grad_affine) against the float64
restatement and the derived bounds of tests/patch_affine_ref.py, and bit for bit against the plain kernels where the
transform is the identity."""
import pytest
import torch

import patch_affine_ref as par

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("u8", "f32")


@pytest.fixture(scope="module")
def table():
    """the shared inputs, the case table and the float64 reference of every case and input kind, computed once"""
    inp = par.inputs()
    cases = par.case_table()
    ref = {}
    for name, tf in cases.items():
        for kind in KINDS:
            img = inp[kind].double() / 255 if kind == "u8" else inp[kind].double()
            ref[name, kind] = (par.composite(img, inp["patch"], tf).detach(),
                               par.gradient(img, inp["patch"], tf, inp["dimg"]))
    dev = {k: v.to(DEV) for k, v in inp.items()}
    return inp, dev, cases, ref


def test_both_kernels_match_float64_on_the_case_table(table):
    """every case, uint8 and f32 input: the composited image and the encoder input within 4 delta_n + 4 * 2^-23 of
    the float64 compositor, the patch gradient within 2 delta_max C_e + (n_e + 8) 2^-24 S_e of its autograd gradient"""
    from sdreamer import kernels as K
    inp, dev, cases, ref = table
    worst = [0.0, 0.0]
    for name, tf in cases.items():
        fb, gb = par.forward_bound(tf), par.gradient_bound(tf, inp["dimg"])
        d_tf = tf.to(DEV)
        grad, tv = K.patch_grad_affine(dev["dimg"], d_tf, (par.PH, par.PW), patch=dev["patch"])
        assert tv.shape == (1,)
        for kind in KINDS:
            f, enc = K.patch_apply_affine(dev[kind], dev["patch"], d_tf)
            assert f.shape == (par.NB, par.H, par.W, par.C) and enc.shape == (par.NB, par.H, par.W, par.CP)
            want, want_g = ref[name, kind]
            ff = float(((f.cpu().double() - want).abs() / fb).max())
            fe = float(((enc[..., :par.C].cpu().double() - (want - 0.5)).abs() / fb).max())
            fg = float(((grad.cpu().double() - want_g).abs() / gb.clamp_min(1e-300)).max())
            print(f"{name:16s} {kind:3s}: image {ff:.3f}, encoder input {fe:.3f}, gradient {fg:.3f} of the bound",
                  flush=True)
            assert not bool(enc[..., par.C:].any())
            assert ff <= 1.0 and fe <= 1.0 and fg <= 1.0, (name, kind, ff, fe, fg)
            worst = [max(worst[0], ff, fe), max(worst[1], fg)]
    print(f"largest used fraction: forward {worst[0]:.3f}, gradient {worst[1]:.3f}", flush=True)


def test_identity_rows_give_the_plain_kernels_bits(table):
    from sdreamer import kernels as K
    inp, dev, cases, _ = table
    tf = cases["identity"]
    offs = par.plain_offsets(tf).to(DEV)
    g = torch.Generator().manual_seed(7)
    anyp = torch.rand(par.PH, par.PW, par.C, generator=g).to(DEV)  # values below 0.25 included
    for patch in (dev["patch"], anyp):
        for kind in KINDS:
            f0, e0 = K.patch_apply(dev[kind], patch, offs)
            f1, e1 = K.patch_apply_affine(dev[kind], patch, tf.to(DEV))
            assert torch.equal(f0, f1) and torch.equal(e0, e1), kind
        d0, tv0 = K.patch_grad(dev["dimg"], offs, (par.PH, par.PW))
        d1, tv1 = K.patch_grad_affine(dev["dimg"], tf.to(DEV), (par.PH, par.PW))
        assert torch.equal(d0, d1) and tv0 is None and tv1 is None
        d0, tv0 = K.patch_grad(dev["dimg"], offs, (par.PH, par.PW), patch=patch, w_tv=0.01)
        d1, tv1 = K.patch_grad_affine(dev["dimg"], tf.to(DEV), (par.PH, par.PW), patch=patch, w_tv=0.01)
        assert torch.equal(d0, d1) and torch.equal(tv0, tv1) and float(tv0) > 0
    assert bool(d0.any())


def test_off_image_rows_leave_the_input_and_give_no_gradient(table):
    from sdreamer import kernels as K
    inp, dev, cases, _ = table
    tf = cases["off_image"].to(DEV)
    f, enc = K.patch_apply_affine(dev["u8"], dev["patch"], tf)
    f0, e0 = K.u8_image_inputs(dev["u8"], par.CP, 0.5)
    assert torch.equal(f, f0) and torch.equal(enc, e0)
    f, _ = K.patch_apply_affine(dev["f32"], dev["patch"], tf)
    assert torch.equal(f, dev["f32"])
    d, tv = K.patch_grad_affine(dev["dimg"], tf, (par.PH, par.PW))
    assert not bool(d.any()) and tv is None
    # with the patch: the TV term alone, as the plain kernel adds it to a zero gradient
    away = torch.tensor([[-100, -100]] * par.NB, dtype=torch.int32, device=DEV)
    d, tv = K.patch_grad_affine(dev["dimg"], tf, (par.PH, par.PW), patch=dev["patch"], w_tv=0.3)
    d0, tv0 = K.patch_grad(dev["dimg"], away, (par.PH, par.PW), patch=dev["patch"], w_tv=0.3)
    assert torch.equal(d, d0) and torch.equal(tv, tv0) and bool(d.any())


@pytest.mark.parametrize("name", ["rotation", "scale2_half_off", "photometric"])
def test_grad_is_the_adjoint_of_apply(table, name):
    """<apply(p + d) - apply(p), g> against <d, grad(g)>, both accumulated in float64 on the host, for a d of half the
    case's clamp margin (no element crosses a kink, so the compositor is affine in d); the bound is the gradient
    bound summed over the elements, and beside it the sharper form weighed by |d| (derived at the assertion)."""
    from sdreamer import kernels as K
    inp, dev, cases, _ = table
    tf = cases[name]
    step = 0.5 * par.margin(inp["patch"], tf) / float(tf[:, 6].abs().max())
    sign = torch.randint(0, 2, inp["patch"].shape, generator=torch.Generator().manual_seed(3)).float() * 2 - 1
    d = (step * sign).to(DEV)
    moved = dev["patch"] + d
    assert float(moved.min()) >= 0 and float(moved.max()) <= 1
    a1, _ = K.patch_apply_affine(dev["f32"], moved, tf.to(DEV))
    a0, _ = K.patch_apply_affine(dev["f32"], dev["patch"], tf.to(DEV))
    grad, _ = K.patch_grad_affine(dev["dimg"], tf.to(DEV), (par.PH, par.PW), patch=dev["patch"])
    d = (moved - dev["patch"]).cpu().double()  # the step as f32 holds it
    lhs = float(((a1.cpu().double() - a0.cpu().double()) * inp["dimg"].double()).sum())
    rhs = float((d * grad.cpu().double()).sum())
    gb = par.gradient_bound(tf, inp["dimg"])
    bound = float(gb.sum())
    # the same bound with each element's share weighed by its |d_e|, plus what the two forwards may round: 4 * 2^-23
    # each (the forward bound's rounding term; their coordinates are the same bits, so delta cancels) at every pixel
    # the patch reaches
    alpha = par.hat_weights(tf)[0].sum(dim=(3, 4))
    tight = float((d.abs() * gb).sum()) + 2 * 4 * 2.0 ** -23 * float(
        (inp["dimg"].double().abs() * (alpha > 0).unsqueeze(-1)).sum())
    print(f"{name}: <dA, g> {lhs:.6e}, <d, grad> {rhs:.6e}, difference {abs(lhs - rhs):.2e} = "
          f"{abs(lhs - rhs) / bound:.2e} of the bound {bound:.2e}, {abs(lhs - rhs) / tight:.3f} of the weighted "
          f"bound {tight:.2e}", flush=True)
    assert abs(lhs - rhs) <= bound
    assert abs(lhs - rhs) <= tight


def test_same_bits_on_repetition(table):
    from sdreamer import kernels as K
    inp, dev, cases, _ = table
    for name in ("rotation", "photometric"):
        tf = cases[name].to(DEV)
        a = K.patch_apply_affine(dev["u8"], dev["patch"], tf)
        b = K.patch_apply_affine(dev["u8"], dev["patch"], tf)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        g0 = K.patch_grad_affine(dev["dimg"], tf, (par.PH, par.PW), patch=dev["patch"], w_tv=0.01)
        g1 = K.patch_grad_affine(dev["dimg"], tf, (par.PH, par.PW), patch=dev["patch"], w_tv=0.01)
        assert torch.equal(g0[0], g1[0]) and torch.equal(g0[1], g1[1])


def test_optional_outputs_and_argument_refusals(table):
    from sdreamer import _native as nat
    from sdreamer import kernels as K
    inp, dev, cases, _ = table
    tf = cases["scale"].to(DEV)
    f, enc = K.patch_apply_affine(dev["u8"], dev["patch"], tf)
    none, enc2 = K.patch_apply_affine(dev["u8"], dev["patch"], tf, need_f32=False)
    assert none is None and torch.equal(enc, enc2)
    _, enc8 = K.patch_apply_affine(dev["f32"], dev["patch"], tf, Cp=8, shift=0.25)
    f32, _ = K.patch_apply_affine(dev["f32"], dev["patch"], tf)
    assert enc8.shape[-1] == 8 and torch.equal(enc8[..., :par.C], f32 - 0.25) and not bool(enc8[..., par.C:].any())
    # img alone (enc NULL) through the C ABI
    img = torch.empty_like(f)
    args = (par.NB, par.H, par.W, par.C, par.CP, par.PH, par.PW, 0.5, K.stream())
    nat.call("sd_patch_apply_affine", K.p(dev["u8"]), 1, K.p(dev["patch"]), K.p(tf), K.p(img), 0, *args)
    assert torch.equal(img, f)
    with pytest.raises(nat.NativeError):  # neither output
        nat.call("sd_patch_apply_affine", K.p(dev["u8"]), 1, K.p(dev["patch"]), K.p(tf), 0, 0, *args)
    with pytest.raises(nat.NativeError):  # no rows
        nat.call("sd_patch_apply_affine", K.p(dev["u8"]), 1, K.p(dev["patch"]), 0, K.p(img), 0, *args)
    with pytest.raises(nat.NativeError):  # Cp < C
        nat.call("sd_patch_apply_affine", K.p(dev["u8"]), 1, K.p(dev["patch"]), K.p(tf), K.p(img), 0, par.NB, par.H,
                 par.W, par.C, 2, par.PH, par.PW, 0.5, K.stream())
    E = par.PH * par.PW * par.C
    dp, part = torch.empty(E, device=DEV), torch.empty(2 * E, device=DEV)
    dims = (par.NB, par.H, par.W, par.C, par.PH, par.PW, K.stream())
    with pytest.raises(nat.NativeError):  # part too small for two chunks
        nat.call("sd_patch_grad_affine", K.p(dev["dimg"]), K.p(tf), K.p(dp), K.p(part), E, 0, 0.0, 0, *dims)
    with pytest.raises(nat.NativeError):  # no rows
        nat.call("sd_patch_grad_affine", K.p(dev["dimg"]), 0, K.p(dp), K.p(part), 2 * E, 0, 0.0, 0, *dims)
    # the Python surface: shapes and dtypes
    with pytest.raises(ValueError):
        K.patch_apply_affine(dev["u8"], dev["patch"], tf[:, :6].contiguous())
    with pytest.raises(ValueError):
        K.patch_apply_affine(dev["u8"], dev["patch"], tf[:-1])
    with pytest.raises(ValueError):
        K.patch_apply_affine(dev["u8"], dev["patch"], tf.double())
    with pytest.raises(ValueError):
        K.patch_apply_affine(dev["u8"], dev["patch"][..., :2].contiguous(), tf)
    with pytest.raises(TypeError):
        K.patch_apply_affine(dev["f32"].double(), dev["patch"], tf)
    with pytest.raises(TypeError):
        K.patch_apply_affine(inp["u8"], dev["patch"], tf)  # a CPU tensor: no fallback
    with pytest.raises(ValueError):
        K.patch_grad_affine(dev["dimg"], tf[:-1], (par.PH, par.PW))
    with pytest.raises(ValueError):
        K.patch_grad_affine(dev["dimg"], tf, (par.PW, par.PH), patch=dev["patch"])
