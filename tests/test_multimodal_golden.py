"""The reference's text-conditioned encoder fixtures (tests/golden/encoder_mm_*.npz, written by gen_golden_mm.py from
the reference's own modules) against the float64 restatement in tests/mm_ref.py, started from the fixture's inputs and
the weights-by-name recipe: pins the fixtures, the recipe and the restatement without the reference."""
import numpy as np
import pytest
import torch

import mm_ref
from golden_io import sample_idx
from test_multimodal_modules import _cnn_cfg


def _rel(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b).max()
    assert err <= 1e-5 * max(np.abs(b).max(), 1e-12), f"{what}: {err} vs scale {np.abs(b).max()}"


def _module(kind, gate):
    from sdreamer.multimodal import GateOnlyEncoder, MultimodalEncoder
    cls = MultimodalEncoder if kind == "mm" else GateOnlyEncoder
    return cls(_cnn_cfg(), (64, 64, 3), use_text_gate=gate)


@pytest.mark.parametrize("name", sorted(mm_ref.CASES))
def test_restatement_reproduces_reference_fixture(name):
    kind, gate = mm_ref.CASES[name]
    z = mm_ref.load_fixture(name)
    sd = mm_ref.fixture_params(_module(kind, gate).state_dict())  # the product's keys / shapes ARE the reference's
    P = mm_ref.f64_params(sd)
    feats = torch.from_numpy(z[f"feat_{int(z['train_text'])}"])
    img = torch.from_numpy(z["image"]).float() / 255.0
    B, T = img.shape[:2]
    visual, gated, g, ctx = mm_ref.encoder_ref(P, feats, img, B, T, kind, gate)
    _rel(ctx[0].numpy(), z["ctx"], "text context")
    _rel(visual.detach().reshape(B, T, -1).numpy(), z["visual_embed"], "visual_embed")
    loss = (visual.reshape(B, T, -1) * torch.from_numpy(z["d_visual"]).double()).sum()
    if gate:
        _rel(gated.detach().reshape(B, T, -1).numpy(), z["rssm_embed"], "rssm_embed")
        _rel(g.mean().item(), z["gate_mean"], "gate mean")
        _rel(g.std().item(), z["gate_std"], "gate std (unbiased)")
        loss = loss + (gated.reshape(B, T, -1) * torch.from_numpy(z["d_rssm"]).double()).sum()
    loss.backward()
    for k, p in P.items():
        key = "encoder." + k
        if k.startswith("text_context_encoder."):
            assert f"gradnone__{key}" in z.files, key  # the reference's update never trains the text front end
            continue
        gr = p.grad.reshape(-1).numpy()
        ref = z[f"grad__{key}"]
        got = gr[sample_idx(key, gr.size)]
        # the fixture's gradients are the reference's float32 autograd: 1e-4 of the largest sampled element
        assert np.abs(got - ref).max() <= 1e-4 * np.abs(ref).max(), key
        assert abs(np.linalg.norm(gr) / float(z[f"gradnorm__{key}"]) - 1) <= 1e-4, key
    # the act shape (no time axis), eval: the first text
    img1 = torch.from_numpy(z["act_image"]).float() / 255.0
    with torch.no_grad():
        visual, gated, _, _ = mm_ref.encoder_ref(P, torch.from_numpy(z["feat_0"]), img1, img1.shape[0], 1, kind, gate)
    _rel(visual.numpy(), z["act_visual_embed"], "act visual_embed")
    if gate:
        _rel(gated.numpy(), z["act_rssm_embed"], "act rssm_embed")
