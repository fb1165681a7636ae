"""Plain-torch float64 restatement of the reference's text-conditioned encoders (text pooling -> FiLM / plain conv
encoder -> text gate), from a reference-layout parameter dict. Shared by the CPU fixture test and the GPU tests."""
import os

import numpy as np
import torch
import torch.nn.functional as F

from oracle import ref_cpu as R
from oracle.init import params_for

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = {"mm_r2": ("mm", True), "mm_filmonly": ("mm", False), "mm_gateonly": ("gateonly", True)}


def load_fixture(name):
    return np.load(os.path.join(GOLDEN, f"encoder_{name}.npz"), allow_pickle=False)


def fixture_params(module_state_dict):
    """the fixture's weights: dense values by name over the reference-layout shapes, checkpoint keys `encoder.*`"""
    vals = params_for({"encoder." + k: tuple(v.shape) for k, v in module_state_dict.items()})
    return {k[len("encoder."):]: torch.from_numpy(v) for k, v in vals.items()}


def f64_params(sd):
    return {k: v.detach().double().cpu().clone().requires_grad_(not k.startswith("text_context_encoder."))
            for k, v in sd.items()}


def text_context(P, feats):
    f = feats.double()
    p = torch.softmax(F.linear(f, P["text_context_encoder.attn_pool.weight"],
                               P["text_context_encoder.attn_pool.bias"]), 0)
    return F.linear((f * p).sum(0, keepdim=True), P["text_context_encoder.proj.weight"],
                    P["text_context_encoder.proj.bias"]).detach()


def encoder_ref(P, feats, img, B, T, kind="mm", gate=True):
    """img float in [0, 1], (B, T, H, W, C) or (B, H, W, C) -> (visual (B*T, E), gated or None, g or None, ctx (1, D))"""
    ctx = text_context(P, feats)
    ce = ctx.expand(B, -1).repeat_interleave(T, 0)
    x = (img.double().reshape(B * T, *img.shape[-3:]) - 0.5).permute(0, 3, 1, 2)
    for i in range(4):
        if kind == "mm":
            cw, cb, nw = (P[f"visual_encoder.convs.{i}.weight"], P[f"visual_encoder.convs.{i}.bias"],
                          P[f"visual_encoder.norms.{i}.weight"])
        else:
            cw, cb, nw = (P[f"conv_encoder.layers.{4 * i}.weight"], P[f"conv_encoder.layers.{4 * i}.bias"],
                          P[f"conv_encoder.layers.{4 * i + 2}.weight"])
        x = R.rms2d(F.max_pool2d(R.conv_same(x, cw, cb), 2, 2), nw)
        if kind == "mm":
            pre = f"visual_encoder.films.{i}.net."
            prm = F.linear(F.silu(F.linear(ce, P[pre + "0.weight"], P[pre + "0.bias"])), P[pre + "2.weight"],
                           P[pre + "2.bias"])
            C = prm.shape[1] // 2
            x = (1 + prm[:, :C])[:, :, None, None] * x + prm[:, C:, None, None]
        x = F.silu(x)
    visual = x.reshape(B * T, -1)
    if not gate:
        return visual, None, None, ctx
    tg = "text_gate."
    tp = F.linear(F.silu(F.linear(ce, P[tg + "text_proj.0.weight"], P[tg + "text_proj.0.bias"])),
                  P[tg + "text_proj.2.weight"], P[tg + "text_proj.2.bias"])
    a = F.linear(F.silu(F.linear(torch.cat([visual, tp], -1), P[tg + "gate_net.0.weight"],
                                 P[tg + "gate_net.0.bias"])), P[tg + "gate_net.2.weight"], P[tg + "gate_net.2.bias"])
    g = torch.sigmoid(a)
    return visual, (1 - g) * visual + g * tp, g, ctx
