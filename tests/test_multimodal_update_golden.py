"""The update-level multimodal fixtures (tests/golden/walker_mm_*.npz, written by gen_golden_mm.py from the reference's
Dreamer) against the float64 restatement in tests/mm_ref.py: text pooling -> FiLM / plain encoder -> gate, started from
the fixture's inputs and the weights-by-name recipe over the fixture's shape table. Pins the fixtures' encoder section,
their forced texts and their seed search without the reference."""
import json
import os

import numpy as np
import pytest
import torch

import mm_ref
from oracle.init import params_for

CASES = {"walker_mm_r2": ("mm", True), "walker_mm_filmonly": ("mm", False), "walker_mm_gateonly": ("gateonly", True)}
FRONT = "encoder.text_context_encoder."


def _rel(a, b, what):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    err = np.abs(a - b).max()
    assert err <= 1e-5 * max(np.abs(b).max(), 1e-12), f"{what}: {err} vs scale {np.abs(b).max()}"


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_reproduces_update_fixture(name):
    kind, gate = CASES[name]
    z = np.load(os.path.join(mm_ref.GOLDEN, name + ".npz"), allow_pickle=False)
    shapes = {k: tuple(v) for k, v in json.loads(str(z["meta_shapes"])).items()}
    vals = params_for(shapes, int(z["meta_param_seed"]))
    P = {k[len("encoder."):]: torch.from_numpy(v).double() for k, v in vals.items() if k.startswith("encoder.")}
    assert int(z["u0_text"]) != int(z["u1_text"])  # the two updates read different texts
    assert float(z["meta_min_gap"]) >= 2e-4 and 0 <= int(z["meta_seed_k"]) <= 50
    # update 0 runs at the recipe's weights (update 1's have moved by one optimizer step)
    img = torch.from_numpy(z["u0_in_image"]).float() / 255.0
    B, T = img.shape[:2]
    feats = torch.from_numpy(z[f"feat_{int(z['u0_text'])}"])
    with torch.no_grad():
        visual, gated, g, ctx = mm_ref.encoder_ref(P, feats, img, B, T, kind, gate)
    _rel(ctx.expand(B, -1).numpy(), z["u0_ctx"], "text context")
    _rel(visual.reshape(B, T, -1).numpy()[..., ::8], z["u0_embed"], "visual_embed")
    if gate:
        _rel(gated.reshape(B, T, -1).numpy()[..., ::8], z["u0_rssm_embed"], "rssm_embed")
        _rel(g.mean().item(), z["u0_gate_mean"], "gate mean")
        _rel(g.std().item(), z["u0_gate_std"], "gate std (unbiased)")
        _rel(g.mean().item(), z["u0_m_encoder/text_gate_mean"], "encoder/text_gate_mean")
    else:
        assert np.array_equal(z["u0_embed"], z["u0_rssm_embed"])
    # the gradient section's context: row b is the context of text b
    with torch.no_grad():
        rows = torch.cat([mm_ref.text_context(P, torch.from_numpy(z[f"feat_{i}"])) for i in (0, 1)])
    _rel(rows.numpy(), z["g_text_ctx"], "per-row text context")
    assert not np.array_equal(z["g_text_ctx"][0], z["g_text_ctx"][1])
    # the text front end: a slot in the shape table, never a gradient, never optimizer state
    front = [k for k in shapes if k.startswith(FRONT)]
    assert len(front) == 4
    for k in front:
        assert f"g_none__{k}" in z.files and f"u0_nostate__{k}" in z.files and f"u1_nostate__{k}" in z.files
    for k in shapes:
        if k not in front:
            assert f"g_{k}__s" in z.files and f"u1_st_{k}__v" in z.files and f"init_{k}__stat" in z.files, k
            assert float(z[f"g_{k}__n"]) > 0, k  # every FiLM, gate and conv tensor gets a gradient
