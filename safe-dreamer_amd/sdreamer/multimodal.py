"""Text-conditioned encoder modules (reference: world_model/multimodal_encoder/, ablations/ablation_encoders.py).

Module trees and parameter names follow the reference, so `state_dict()` keys and reference-layout shapes match
(conv weights convert as networks.Conv2d does). The product never runs CLIP: the frozen token features
(`last_hidden_state`, one (N_tok, clip_dim) array per text) are user data given to `set_text_features`; everything
trainable runs on the HIP kernels:

  * FiLMConvEncoder: ConvEncoder's fused stage kernels with gamma * x + beta in their epilogue
    (ops.ConvPoolNormFn with gamma, beta; one row per batch row, looked up per image);
  * TextGate: out = (1 - g) v + g tp[b], the concatenation cat[v, tp] never materialised (ops.GateFirstFn splits
    gate_net.0.weight into its v and tp halves, the tp half a B-row GEMM added per batch row);
  * TextContextEncoder: attention pooling over the token features (one kernel) + proj, eagerly, into a persistent
    (B, text_context_dim) buffer that captured graphs read — switching text never needs a re-capture.

The text front end (attn_pool, proj) receives no gradient in the reference's update (the context is detached before
the loss): its four tensors are frozen parameters here.
"""
from __future__ import annotations

import random

import numpy as np
import torch
from torch import nn

from . import kernels as K
from . import ops
from .networks import Act, Conv2d, ConvEncoder, Linear, RMSNorm, check_stage_widths, run_conv_stages

TEXT_RESAMPLE_INTERVAL = 64  # training forwards between two text draws (encoder.py:121)


def _xavier_zero_bias(lin):
    with torch.no_grad():
        nn.init.xavier_uniform_(lin.weight)
        if lin.bias is not None:
            lin.bias.zero_()


def _two_layer(inp, hidden, out):
    """nn.Sequential(Linear, SiLU, Linear) with the reference's indices 0 / 2"""
    return nn.Sequential(Linear(inp, hidden), Act(), Linear(hidden, out))


def _mlp2(seq, x):
    h = ops.rowbias_silu(ops.linear(x, seq[0].weight, seq[0].bias))
    return ops.linear(h, seq[2].weight, seq[2].bias)


class FiLMGenerator(nn.Module):
    """visual_encoder.py:17-59: (gamma - 1, beta) = Linear(2C, 2C)(SiLU(Linear(ctx_dim, 2C)(ctx))), the last layer
    zero-initialised (identity modulation at initialisation)."""

    def __init__(self, text_context_dim, num_channels):
        super().__init__()
        self.num_channels = int(num_channels)
        self.net = _two_layer(text_context_dim, 2 * self.num_channels, 2 * self.num_channels)
        _xavier_zero_bias(self.net[0])
        with torch.no_grad():
            self.net[2].weight.zero_()
            self.net[2].bias.zero_()

    def forward(self, ctx):
        """ctx (B, ctx_dim) -> gamma, beta (B, C) contiguous"""
        params = _mlp2(self.net, ctx)
        C = self.num_channels
        return params[:, :C] + 1.0, params[:, C:].contiguous()


class FiLMConvEncoder(nn.Module):
    """visual_encoder.py:63-134: ConvEncoder's stages with FiLM between the norm and the SiLU. Input NHWC
    (B*T, H, W, C) already shifted by -0.5 (channels zero-padded to a multiple of 4, as MultiEncoder forms it);
    output (B*T, C*h*w) in NCHW flatten order."""

    def __init__(self, config, input_shape, text_context_dim):
        super().__init__()
        h, w, ch = input_shape
        self.depths = tuple(int(config.depth) * int(m) for m in list(config.mults))
        check_stage_widths(self.depths)
        self.k = int(config.kernel_size)
        if not bool(config.norm):
            raise NotImplementedError("norm=False encoder")
        self.convs, self.norms, self.films = nn.ModuleList(), nn.ModuleList(), nn.ModuleList()
        inp = ch
        for d in self.depths:
            self.convs.append(Conv2d(inp, d, self.k))
            self.norms.append(RMSNorm(d))
            self.films.append(FiLMGenerator(text_context_dim, d))
            inp = d
            h, w = h // 2, w // 2
        self.out_dim = self.depths[-1] * h * w

    def dgrad_weights(self):
        return [self.convs[i].weight for i in range(1, len(self.depths))]

    def forward(self, x, ctx, split=None, pad_shift=None):
        """ctx (B, ctx_dim), one row per x.shape[0] // B consecutive images. split, pad_shift: see
        networks.run_conv_stages."""
        return run_conv_stages(x, list(zip(self.convs, self.norms, self.films)), split, pad_shift, ctx)


class TextGate(nn.Module):
    """text_encoder.py:134-195: tp = text_proj(ctx); g = sigmoid(gate_net(cat[v, tp])); out = (1 - g) v + g tp."""

    def __init__(self, embed_dim, text_context_dim, gate_init_bias=-3.0):
        super().__init__()
        self.embed_dim = E = int(embed_dim)
        self.text_proj = _two_layer(text_context_dim, E, E)
        self.gate_net = _two_layer(2 * E, E, E)
        for lin in (self.text_proj[0], self.text_proj[2], self.gate_net[0]):
            _xavier_zero_bias(lin)
        with torch.no_grad():
            self.gate_net[2].weight.zero_()
            self.gate_net[2].bias.fill_(float(gate_init_bias))

    def forward(self, v, ctx):
        """v (N, E), ctx (B, ctx_dim) with N % B == 0 (row b holds images b * N/B ..) -> (gated (N, E), g (N, E))"""
        N, B = v.shape[0], ctx.shape[0]
        if N % B:
            raise ValueError(f"{N} embed rows for {B} context rows")
        T = N // B
        tp = _mlp2(self.text_proj, ctx)  # (B, E): never expanded to (N, E)
        h = ops.GateFirstFn.apply(v, tp, self.gate_net[0].weight, self.gate_net[0].bias, T)
        a = ops.linear(h, self.gate_net[2].weight, self.gate_net[2].bias)
        return ops.text_gate(v, a, tp, T)


class TextContextEncoder(nn.Module):
    """text_encoder.py:21-128 without CLIP: attention pooling over the given token features, then proj."""

    def __init__(self, text_context_dim=256, clip_dim=512):
        super().__init__()
        self.clip_dim, self.text_context_dim = int(clip_dim), int(text_context_dim)
        self.attn_pool = Linear(self.clip_dim, 1)
        self.proj = Linear(self.clip_dim, self.text_context_dim)
        _xavier_zero_bias(self.attn_pool)
        _xavier_zero_bias(self.proj)
        for p in self.parameters():  # no gradient ever reaches them (see the module docstring)
            p.requires_grad_(False)

    @torch.no_grad()
    def forward(self, feats, out=None):
        """feats (N_tok, clip_dim) device tensor -> (1, text_context_dim); `out` (B, dim): every row is overwritten
        with the context (a persistent buffer: its address stays put for captured graphs)."""
        if feats.dim() != 2 or feats.shape[1] != self.clip_dim:
            raise ValueError(f"token features must be (N_tok, {self.clip_dim}), got {tuple(feats.shape)}")
        pooled = K.text_pool(feats.contiguous(), self.attn_pool.weight, self.attn_pool.bias)
        ctx = K.linear(pooled, self.proj.weight, self.proj.bias)
        if out is not None:
            out.copy_(ctx.expand_as(out))
            return out
        return ctx


class _TextConditioned(nn.Module):
    """Text bookkeeping shared by MultimodalEncoder and GateOnlyEncoder (encoder.py:144-187): the text pool, the
    draw every TEXT_RESAMPLE_INTERVAL training forwards, the first text in eval, the context cache."""

    def _init_text(self, seed_base=0):
        self._texts, self._feats = None, None
        self._task_name = None
        self._seed_base = int(seed_base)
        self._forward_count = 0
        self._resamples = 0
        self._text_index = None  # the schedule's current text
        self._resume = False  # set by load_text_schedule_state: the first buffer after a resume keeps its text
        self._cached_index = None  # the text whose context the buffer holds
        self._ctx = None  # persistent (B, text_context_dim) buffer
        self._last_gate = None
        # act()'s own cache and schedule (the reference's frozen copy keeps its own): never the update's buffer, whose
        # address the update graphs hold
        self._act = dict(ctx=None, cached=None, index=None, forwards=0, draws=0)
        self.cnn_shapes, self.mlp_shapes = {"image": None}, {}  # MultiEncoder's key tables (Dreamer.preprocess / act)
        self.register_load_state_dict_post_hook(lambda module, incompatible: module.invalidate_text_cache())

    def set_text_features(self, texts, feats):
        """texts: list of strings; feats[i]: (N_tok_i, clip_dim) array or tensor, the frozen text model's
        last_hidden_state for texts[i]."""
        texts = list(texts)
        if not texts or len(texts) != len(feats):
            raise ValueError("set_text_features needs one (N_tok, clip_dim) feature array per text, at least one")
        conv = []
        for f in feats:
            t = torch.as_tensor(np.asarray(f) if not torch.is_tensor(f) else f, dtype=torch.float32)
            if t.dim() == 3 and t.shape[0] == 1:
                t = t[0]
            if t.dim() != 2 or t.shape[1] != self.text_context_encoder.clip_dim or not 1 <= t.shape[0] <= 128:
                raise ValueError(f"token features must be (N_tok <= 128, {self.text_context_encoder.clip_dim}), got "
                                 f"{tuple(t.shape)}")
            conv.append(t.contiguous())
        self._texts, self._feats = texts, conv
        self.invalidate_text_cache()

    def load_text_features(self, path):
        """an .npz with `texts` (array of strings) and `feat_<i>` per text"""
        z = np.load(path, allow_pickle=False)
        texts = [str(t) for t in z["texts"]]
        self.set_text_features(texts, [z[f"feat_{i}"] for i in range(len(texts))])

    def _need_features(self):
        if self._feats is None:
            raise ValueError("the multimodal encoder has no text features: call set_text_features(texts, feats) or set "
                             "model.multimodal_encoder.text_features to an .npz (the product never runs CLIP)")

    def set_task_name(self, task_name):
        self._need_features()
        self._task_name = str(task_name)

    def _next_text(self, fresh=False):
        """Host-side schedule (encoder.py:150-187): the index of the text this forward uses. Training: a new draw on
        the first forward, when the context buffer is new (`fresh`) and every TEXT_RESAMPLE_INTERVAL forwards, seeded
        from (seed base, number of draws so far) so a run repeats; eval: the first text."""
        self._need_features()
        if not self.training:
            return 0
        if self._resume:  # resumed mid-interval: a new buffer, but not a new draw
            fresh, self._resume = False, False
        if self._text_index is None or fresh or self._forward_count % TEXT_RESAMPLE_INTERVAL == 0:
            self._text_index = random.Random(self._seed_base * 1000003 + self._resamples).randrange(len(self._texts))
            self._resamples += 1
        self._forward_count += 1
        return self._text_index

    def text_schedule_state(self):
        """the update-side schedule as plain ints (checkpoint resume); -1: no text drawn yet"""
        return {"forwards": int(self._forward_count), "draws": int(self._resamples),
                "index": -1 if self._text_index is None else int(self._text_index)}

    def load_text_schedule_state(self, st):
        self._forward_count, self._resamples = int(st["forwards"]), int(st["draws"])
        self._text_index = None if int(st["index"]) < 0 else int(st["index"])
        self._resume = self._text_index is not None  # the first context buffer after a resume keeps this text

    def invalidate_text_cache(self):
        """the next forward recomputes its context into the same buffer (new features or attn_pool / proj weights)"""
        self._cached_index = None
        self._act["cached"] = None

    def act_context(self, B, device, eval=False):
        """text_context for Dreamer.act: its own (B, dim) buffer, eval -> the first text, else its own 64-forward
        schedule (draws seeded apart from the update's). While a graph is being captured nothing is computed: the
        buffer prepared before the capture is returned, and refreshed eagerly before every replay."""
        self._need_features()
        a = self._act
        if torch.cuda.is_current_stream_capturing():
            if a["ctx"] is None or a["ctx"].shape[0] != B:
                raise RuntimeError("act_context must be prepared before a graph capture")
            return a["ctx"]
        fresh = a["ctx"] is None or a["ctx"].shape[0] != B
        if eval:
            idx = 0
        else:
            if a["index"] is None or fresh or a["forwards"] % TEXT_RESAMPLE_INTERVAL == 0:
                a["index"] = random.Random(self._seed_base * 1000003 + 500009 + a["draws"]).randrange(len(self._texts))
                a["draws"] += 1
            a["forwards"] += 1
            idx = a["index"]
        if fresh:
            a["ctx"] = torch.empty(B, self.text_context_encoder.text_context_dim, dtype=torch.float32, device=device)
        if fresh or idx != a["cached"]:
            self.text_context_encoder(self._feats[idx].to(device), out=a["ctx"])
            a["cached"] = idx
        return a["ctx"]

    def text_context(self, B, device, force_index=None):
        """(B, text_context_dim) context of the current text; eager (outside any captured graph). The buffer keeps
        its address while B and the device stay the same."""
        self._need_features()
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:  # "cuda" names the current device
            device = torch.device("cuda", torch.cuda.current_device())
        fresh = self._ctx is None or self._ctx.shape[0] != B or self._ctx.device != device
        idx = int(force_index) if force_index is not None else self._next_text(fresh)
        if fresh:
            self._ctx = torch.empty(B, self.text_context_encoder.text_context_dim, dtype=torch.float32, device=device)
        if fresh or idx != self._cached_index:
            self.text_context_encoder(self._feats[idx].to(device), out=self._ctx)
            self._cached_index = idx
        return self._ctx

    def gate_metrics(self):
        """the gate's mean / unbiased std as lazy metrics (K.Stat: resolved with the update's others, no host sync)"""
        if self._last_gate is None:
            return {}
        return {"encoder/text_gate_mean": K.Stat(self._last_gate, K.STAT_MEAN),
                "encoder/text_gate_std": K.Stat(self._last_gate, K.STAT_STD)}

    def weight_diagnostics(self):
        """get_diagnostics' three weight figures (encoder.py:269-275) as 0-dim device tensors: no host sync. Read after
        the optimizer step, as the reference reads them."""
        if not self._use_text_gate:
            return {}
        last, proj = self.text_gate.gate_net[2], self.text_gate.text_proj
        with torch.no_grad():
            return {"encoder/text_gate_final_bias_mean": last.bias.mean(),
                    "encoder/text_gate_final_weight_norm": torch.linalg.vector_norm(last.weight),
                    "encoder/text_proj_weight_norm": torch.linalg.vector_norm(proj[0].weight) +
                    torch.linalg.vector_norm(proj[2].weight)}

    def _images(self, obs):
        """obs['image'] (B, T, H, W, C) or (B, H, W, C) float in [0, 1] -> (x (N, H, W, Cp) shifted by -0.5, B, T,
        has_time, pad_shift). pad_shift 0.5: x is the raw image, whose gradient is wanted; the first stage shifts and
        pads it itself (ConvEncoder.forward)."""
        pre = obs.get("__enc_image")  # formed by Dreamer.preprocess(enc_input=True) from the uint8 bytes
        img = pre if pre is not None else obs["image"]
        has_time = img.dim() == 5
        B, T = (img.shape[0], img.shape[1]) if has_time else (img.shape[0], 1)
        x = img.reshape(-1, *img.shape[-3:]).contiguous()
        pad_shift = None
        if pre is not None:
            pass
        elif x.shape[-1] % 4 and x.requires_grad and torch.is_grad_enabled():
            pad_shift = 0.5
        elif x.shape[-1] % 4:
            x = K.pad_channels(x, (x.shape[-1] + 3) // 4 * 4, 0.5)
        else:
            x = x - 0.5
        return x, B, T, has_time, pad_shift

    def _finish(self, visual, ctx, B, T, has_time, return_both):
        shape = (B, T, -1) if has_time else (B, -1)
        if not (return_both and self._use_text_gate):
            return visual.reshape(*shape)
        gated, g = self.text_gate(visual, ctx)
        if torch.is_grad_enabled():  # the update's forward; act / video_pred (no_grad) leave its diagnostic alone
            self._last_gate = g.detach()
        return visual.reshape(*shape), gated.reshape(*shape)


class MultimodalEncoder(_TextConditioned):
    """encoder.py:62-284: FiLM-conditioned visual encoder + optional text gate. forward returns
    (visual_embed, rssm_embed) — visual_embed the pure visual target of Barlow / InfoNCE, rssm_embed the gated input
    of the RSSM — or visual_embed alone without the gate / with return_both=False."""

    def __init__(self, cnn_config, input_shape, text_context_dim=256, clip_dim=512, use_text_gate=True,
                 gate_init_bias=-3.0, seed_base=0):
        super().__init__()
        self._use_text_gate = bool(use_text_gate)
        self.text_context_encoder = TextContextEncoder(text_context_dim, clip_dim)
        self.visual_encoder = FiLMConvEncoder(cnn_config, input_shape, text_context_dim)
        self.out_dim = self.visual_encoder.out_dim
        if self._use_text_gate:
            self.text_gate = TextGate(self.out_dim, text_context_dim, gate_init_bias)
        self._init_text(seed_base)

    def dgrad_weights(self):
        return self.visual_encoder.dgrad_weights()

    def forward(self, obs, return_both=True, reuse_text_context=None, split=None):
        x, B, T, has_time, pad_shift = self._images(obs)
        ctx = reuse_text_context if reuse_text_context is not None else self.text_context(B, x.device)
        visual = self.visual_encoder(x, ctx, split, pad_shift)
        return self._finish(visual, ctx, B, T, has_time, return_both)


class GateOnlyEncoder(_TextConditioned):
    """ablation_encoders.py:37-163: the plain ConvEncoder (keys conv_encoder.*) followed by the TextGate."""

    def __init__(self, cnn_config, input_shape, text_context_dim=256, clip_dim=512, use_text_gate=True,
                 gate_init_bias=-3.0, seed_base=0):
        super().__init__()
        self._use_text_gate = bool(use_text_gate)
        self.conv_encoder = ConvEncoder(cnn_config, input_shape)
        self.out_dim = self.conv_encoder.out_dim
        self.text_context_encoder = TextContextEncoder(text_context_dim, clip_dim)
        if self._use_text_gate:
            self.text_gate = TextGate(self.out_dim, text_context_dim, gate_init_bias)
        self._init_text(seed_base)

    def dgrad_weights(self):
        return self.conv_encoder.dgrad_weights()

    def forward(self, obs, return_both=True, reuse_text_context=None, split=None):
        x, B, T, has_time, pad_shift = self._images(obs)
        visual = self.conv_encoder(x, split, pad_shift)
        ctx = None
        if return_both and self._use_text_gate:
            ctx = reuse_text_context if reuse_text_context is not None else self.text_context(B, x.device)
        return self._finish(visual, ctx, B, T, has_time, return_both)


class MLPProjector(nn.Module):
    """networks.py:390-403: fc1 -> nn.RMSNorm(out) -> SiLU -> fc2, no biases. nn.RMSNorm(out) has eps=None: float32
    machine epsilon in the f32 run, not the 1e-4 of every other norm."""

    EPS = float(torch.finfo(torch.float32).eps)

    def __init__(self, in_ch, out_ch):
        super().__init__()
        self.fc1 = Linear(in_ch, out_ch, bias=False)
        self.norm = RMSNorm(out_ch, eps=self.EPS)
        self.fc2 = Linear(out_ch, out_ch, bias=False)

    def forward(self, x):
        h = ops.rms_silu(ops.linear(x, self.fc1.weight, None), self.norm.weight, eps=self.EPS)
        return ops.linear(h, self.fc2.weight, None)
