"""The adversarial patch kernels (csrc/attack.hip): sd_patch_apply, sd_patch_grad, sd_patch_step."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
NB, H, W, C, PH, PW = 5, 64, 64, 3, 16, 16
# inside; negative row; past the bottom-right border; negative column; entirely outside (contributes nothing)
OFFS = [(24, 24), (-5, 10), (60, 55), (20, -7), (100, 100)]


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _offs():
    return torch.tensor(OFFS, dtype=torch.int32)


def _window_mask():
    m = torch.zeros(NB, H, W, dtype=torch.bool)
    for n, (oy, ox) in enumerate(OFFS):
        m[n, max(oy, 0):max(min(oy + PH, H), 0), max(ox, 0):max(min(ox + PW, W), 0)] = True
    return m


def _apply_ref(img, patch):
    out = img.clone()
    for n, (oy, ox) in enumerate(OFFS):
        for py in range(PH):
            for px in range(PW):
                y, x = oy + py, ox + px
                if 0 <= y < H and 0 <= x < W:
                    out[n, y, x] = patch[py, px]
    return out


def test_patch_apply_composites_and_forms_the_encoder_input():
    from sdreamer import kernels as K
    img = torch.rand(NB, H, W, C, generator=_g(1))
    patch = torch.rand(PH, PW, C, generator=_g(2))
    f, enc = K.patch_apply(img.to(DEV), patch.to(DEV), _offs().to(DEV))
    ref = _apply_ref(img, patch)
    assert torch.equal(f.cpu(), ref)
    assert enc.shape == (NB, H, W, 4)
    assert torch.equal(enc[..., :3].cpu(), ref - 0.5)
    assert torch.equal(enc[..., 3].cpu(), torch.zeros(NB, H, W))
    assert torch.equal(f[4].cpu(), img[4])  # the window entirely outside the image
    none, enc2 = K.patch_apply(img.to(DEV), patch.to(DEV), _offs().to(DEV), need_f32=False)
    assert none is None and torch.equal(enc2, enc)


def test_patch_apply_uint8_equals_u8_image_inputs_off_the_patch():
    from sdreamer import kernels as K
    u8 = torch.randint(0, 256, (NB, H, W, C), generator=_g(3), dtype=torch.uint8).to(DEV)
    patch = torch.rand(PH, PW, C, generator=_g(4)).to(DEV)
    f0, e0 = K.u8_image_inputs(u8, 4, 0.5)
    f, e = K.patch_apply(u8, patch, _offs().to(DEV))
    off = ~_window_mask().to(DEV)
    assert torch.equal(f[off], f0[off]) and torch.equal(e[off], e0[off])
    away = torch.full((NB, 2), 1000, dtype=torch.int32, device=DEV)
    f1, e1 = K.patch_apply(u8, patch, away)
    assert torch.equal(f1, f0) and torch.equal(e1, e0)
    assert torch.equal(f.cpu(), _apply_ref(f0.cpu(), patch.cpu()))


def test_patch_grad_is_the_adjoint_of_apply():
    """<apply(p) - apply(0), G> = <p, patch_grad(G)> with both inner products accumulated in float64 on the host, to
    1e-6 relative; the image whose window lies outside contributes nothing; a repeated call is bit-identical."""
    from sdreamer import kernels as K
    img = torch.rand(NB, H, W, C, generator=_g(5)).to(DEV)
    patch = torch.rand(PH, PW, C, generator=_g(6)).to(DEV)
    G = torch.randn(NB, H, W, C, generator=_g(7)).to(DEV)
    offs = _offs().to(DEV)
    a1, _ = K.patch_apply(img, patch, offs)
    a0, _ = K.patch_apply(img, torch.zeros_like(patch), offs)
    d, tv = K.patch_grad(G, offs, (PH, PW))
    assert tv is None and d.shape == (PH, PW, C)
    lhs = float(((a1.double() - a0.double()).cpu() * G.double().cpu()).sum())
    rhs = float((patch.double().cpu() * d.double().cpu()).sum())
    print(f"patch adjointness: lhs {lhs:.9e} rhs {rhs:.9e} rel {abs(lhs - rhs) / abs(lhs):.2e}")
    assert abs(lhs - rhs) <= 1e-6 * abs(lhs)
    d2, _ = K.patch_grad(G, offs, (PH, PW))
    assert torch.equal(d, d2)
    only_out = torch.zeros_like(G)
    only_out[4] = G[4]
    z, _ = K.patch_grad(only_out, offs, (PH, PW))
    assert torch.equal(z, torch.zeros_like(z))
    # more images than one reduction chunk (two stages), against the float64 sum
    nb = 70
    Gb = torch.randn(nb, H, W, C, generator=_g(8))
    ob = torch.randint(-20, 70, (nb, 2), generator=_g(9), dtype=torch.int32)
    db, _ = K.patch_grad(Gb.to(DEV), ob.to(DEV), (PH, PW))
    ref = torch.zeros(PH, PW, C, dtype=torch.float64)
    mag = torch.zeros(PH, PW, C, dtype=torch.float64)
    for n in range(nb):
        oy, ox = int(ob[n, 0]), int(ob[n, 1])
        y0, y1, x0, x1 = max(oy, 0), min(oy + PH, H), max(ox, 0), min(ox + PW, W)
        if y1 > y0 and x1 > x0:
            ref[y0 - oy:y1 - oy, x0 - ox:x1 - ox] += Gb[n, y0:y1, x0:x1].double()
            mag[y0 - oy:y1 - oy, x0 - ox:x1 - ox] += Gb[n, y0:y1, x0:x1].double().abs()
    assert float(((db.cpu().double() - ref).abs() - 1e-6 * mag).max()) <= 0
    assert torch.equal(db, K.patch_grad(Gb.to(DEV), ob.to(DEV), (PH, PW))[0])


def test_patch_total_variation_matches_autograd():
    """TV value and gradient against torch autograd on the CPU: the gradient is a sum of at most four signs times
    w_tv (exact up to one rounding: 1e-6), the value an f32 sum of ~1.4k terms (1e-5 relative)."""
    from sdreamer import kernels as K
    patch = torch.rand(PH, PW, C, generator=_g(10))
    patch[3, 4] = patch[3, 5]  # a zero difference: sign(0) = 0, as torch's abs backward
    G = torch.zeros(NB, H, W, C, device=DEV)
    w_tv = 0.01
    p = patch.clone().requires_grad_()
    tv_ref = (p[:, 1:] - p[:, :-1]).abs().sum() + (p[1:] - p[:-1]).abs().sum()
    tv_ref.backward()
    d, tv = K.patch_grad(G, _offs().to(DEV), (PH, PW), patch=patch.to(DEV), w_tv=w_tv)
    assert abs(float(tv) - float(tv_ref.detach())) <= 1e-5 * float(tv_ref.detach())
    assert float((d.cpu() - w_tv * p.grad).abs().max()) <= 1e-6
    Gr = torch.randn(NB, H, W, C, generator=_g(11)).to(DEV)
    d0, _ = K.patch_grad(Gr, _offs().to(DEV), (PH, PW))
    d1, _ = K.patch_grad(Gr, _offs().to(DEV), (PH, PW), patch=patch.to(DEV), w_tv=w_tv)
    assert float((d1.cpu() - (d0.cpu() + w_tv * p.grad)).abs().max()) <= 1e-6


def _adam_ref(p0, grads, lr, base=None, eps=None):
    p = p0.clone().requires_grad_()
    opt = torch.optim.Adam([p], lr=lr)
    for g in grads:
        p.grad = g.clone()
        opt.step()
        with torch.no_grad():
            p.clamp_(0.0, 1.0)
            if eps is not None:
                e = torch.tensor(eps, dtype=torch.float32)
                p.copy_(torch.min(torch.max(p, base - e), base + e))
    return p.detach()


def test_patch_step_matches_adam_and_projects():
    from sdreamer import kernels as K
    p0 = torch.rand(PH, PW, C, generator=_g(12))
    grads = [torch.randn(PH, PW, C, generator=_g(13 + i)) for i in range(3)]
    ref = _adam_ref(p0, grads, 0.05)
    p = p0.to(DEV)
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    for g in grads:
        K.patch_step(p, g.to(DEV), m, v, step, 0.05)
    assert int(step) == 3
    assert float((p.cpu() - ref).abs().max()) <= 1e-6
    assert float(p.min()) >= 0.0 and float(p.max()) <= 1.0
    # L-inf ball around a base patch: a large step puts most elements on a face, exactly
    base = 0.2 + 0.6 * torch.rand(PH, PW, C, generator=_g(20))
    eps = 0.03
    ref = _adam_ref(base, grads, 0.5, base=base, eps=eps)
    p = base.to(DEV).clone()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    step = torch.zeros(1, dtype=torch.int32, device=DEV)
    for g in grads:
        K.patch_step(p, g.to(DEV), m, v, step, 0.5, base=base.to(DEV), eps=eps)
    e = torch.tensor(eps, dtype=torch.float32)
    lo, hi = base - e, base + e
    got = p.cpu()
    assert bool(((got >= lo) & (got <= hi)).all())
    face = (ref == lo) | (ref == hi)
    assert int(face.sum()) > face.numel() // 2
    assert torch.equal(got[face], ref[face])
    assert float((got - ref).abs().max()) <= 1e-6
