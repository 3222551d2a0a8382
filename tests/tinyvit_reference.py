"""CPU fp32 reference of the TinyViT encoder for the tests: a ``torch.nn`` module built from Conv2d / BatchNorm2d /
LayerNorm / Linear / GELU under timm's module names (``patch_embed.conv1.conv``, ``stages_1.blocks.0.attn.qkv``, ...),
so its ``state_dict`` has the checkpoint keys the reference's student model carries under ``image_encoder.model.``.

``emulate_bf16=True`` rounds at the points csrc/tinyvit.hip rounds (DESIGN.md "TinyViT encoder"): the frames, every
GEMM weight after BatchNorm folding, and every layer output (stem convs, MBConv convs, PatchMerging convs, LayerNorm
outputs, qkv, the attention context, residual sums, local_conv, fc1).  Depthwise weights, biases, LayerNorm
parameters, attention biases, softmax and every accumulation stay fp32.  ``dtype=torch.float64`` runs the same
rounding points with fp64 accumulation: the gap between the two measures what a different summation order costs."""
from __future__ import annotations

import itertools
from typing import Dict, List

import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from gitcap.tinyvit_config import TinyViTConfig, fold_convnorm


def _bf(x: torch.Tensor) -> torch.Tensor:
    return x.to(torch.bfloat16).to(x.dtype)


def attention_bias_idxs(ws: int) -> torch.Tensor:
    """[N, N] index of (|dy|, |dx|) in order of first appearance over points x points, row-major (timm's rule)."""
    points = list(itertools.product(range(ws), range(ws)))
    offsets: Dict[tuple, int] = {}
    idxs = []
    for p1 in points:
        for p2 in points:
            off = (abs(p1[0] - p2[0]), abs(p1[1] - p2[1]))
            if off not in offsets:
                offsets[off] = len(offsets)
            idxs.append(offsets[off])
    return torch.tensor(idxs, dtype=torch.long).view(len(points), len(points))


class _Ctx:
    emu = False

    def r(self, x):
        return _bf(x) if self.emu else x


class ConvNorm(nn.Module):
    def __init__(self, cin, cout, k=1, stride=1, pad=0, groups=1):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride, pad, groups=groups, bias=False)
        self.bn = nn.BatchNorm2d(cout)
        self.stride, self.pad, self.groups = stride, pad, groups

    def run(self, x, ctx: _Ctx):
        if not ctx.emu:
            return self.bn(self.conv(x))
        w, b = fold_convnorm(self.conv.weight.detach().numpy(), self.bn.weight.detach().numpy(), self.bn.bias.detach().numpy(),
                             self.bn.running_mean.numpy(), self.bn.running_var.numpy(), self.bn.eps)
        w, b = torch.from_numpy(w).to(x.dtype), torch.from_numpy(b).to(x.dtype)
        if self.groups == 1:
            w = _bf(w)                  # GEMM weights are bf16 on the device; depthwise weights stay fp32
        return F.conv2d(x, w, b, self.stride, self.pad, groups=self.groups)


def _lin(m: nn.Linear, x, ctx: _Ctx):
    w = m.weight.to(x.dtype)
    return F.linear(x, _bf(w) if ctx.emu else w, m.bias.to(x.dtype))


class PatchEmbed(nn.Module):
    def __init__(self, c0):
        super().__init__()
        self.conv1 = ConvNorm(3, c0 // 2, 3, 2, 1)
        self.conv2 = ConvNorm(c0 // 2, c0, 3, 2, 1)

    def run(self, x, ctx):
        x = ctx.r(F.gelu(self.conv1.run(ctx.r(x), ctx)))
        return ctx.r(self.conv2.run(x, ctx))


class MBConv(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.conv1 = ConvNorm(c, 4 * c)
        self.conv2 = ConvNorm(4 * c, 4 * c, 3, 1, 1, groups=4 * c)
        self.conv3 = ConvNorm(4 * c, c)

    def run(self, x, ctx):
        h = ctx.r(F.gelu(self.conv1.run(x, ctx)))
        h = ctx.r(F.gelu(self.conv2.run(h, ctx)))
        return ctx.r(F.gelu(x + self.conv3.run(h, ctx)))        # act3 after the residual add


class PatchMerging(nn.Module):
    def __init__(self, cin, cout, stride):
        super().__init__()
        self.conv1 = ConvNorm(cin, cout)
        self.conv2 = ConvNorm(cout, cout, 3, stride, 1, groups=cout)
        self.conv3 = ConvNorm(cout, cout)

    def run(self, x, ctx):
        x = ctx.r(F.gelu(self.conv1.run(x, ctx)))
        x = ctx.r(F.gelu(self.conv2.run(x, ctx)))
        return ctx.r(self.conv3.run(x, ctx))


class Attention(nn.Module):
    def __init__(self, c, heads, ws):
        super().__init__()
        self.heads, self.ws = heads, ws
        self.norm = nn.LayerNorm(c, eps=1e-5)
        self.qkv = nn.Linear(c, 3 * c)
        self.proj = nn.Linear(c, c)
        self.attention_biases = nn.Parameter(torch.zeros(heads, ws * ws))
        self.register_buffer("attention_bias_idxs", attention_bias_idxs(ws), persistent=False)

    def bias(self) -> torch.Tensor:                     # [heads, N, N]
        return self.attention_biases[:, self.attention_bias_idxs]

    def run(self, x, ctx):                              # x [B', N, C] -> proj output (unrounded: the residual add rounds)
        Bw, N, C = x.shape
        xn = ctx.r(F.layer_norm(x, (C,), self.norm.weight.to(x.dtype), self.norm.bias.to(x.dtype), self.norm.eps))
        qkv = ctx.r(_lin(self.qkv, xn, ctx))
        q, k, v = qkv.view(Bw, N, self.heads, -1).split([32, 32, 32], dim=3)    # per-head interleaved
        q, k, v = (t.permute(0, 2, 1, 3) for t in (q, k, v))
        a = (q @ k.transpose(-2, -1)) * (32 ** -0.5) + self.bias().to(x.dtype)
        o = a.softmax(dim=-1) @ v
        o = ctx.r(o.transpose(1, 2).reshape(Bw, N, C))
        return _lin(self.proj, o, ctx)


class NormMlp(nn.Module):
    def __init__(self, c):
        super().__init__()
        self.norm = nn.LayerNorm(c, eps=1e-5)
        self.fc1 = nn.Linear(c, 4 * c)
        self.fc2 = nn.Linear(4 * c, c)

    def run(self, x, ctx):
        C = x.shape[-1]
        xn = ctx.r(F.layer_norm(x, (C,), self.norm.weight.to(x.dtype), self.norm.bias.to(x.dtype), self.norm.eps))
        return _lin(self.fc2, ctx.r(F.gelu(_lin(self.fc1, xn, ctx))), ctx)


class TinyVitBlock(nn.Module):
    def __init__(self, c, heads, ws):
        super().__init__()
        self.ws = ws
        self.attn = Attention(c, heads, ws)
        self.local_conv = ConvNorm(c, c, 3, 1, 1, groups=c)
        self.mlp = NormMlp(c)

    def run(self, x, ctx):                              # x [B, H, W, C]
        B, H, W, C = x.shape
        ws = self.ws
        nH, nW = H // ws, W // ws
        t = x.view(B, nH, ws, nW, ws, C).transpose(2, 3).reshape(B * nH * nW, ws * ws, C)
        t = self.attn.run(t, ctx)
        t = t.view(B, nH, nW, ws, ws, C).transpose(2, 3).reshape(B, H, W, C)
        x = ctx.r(x + t)
        x = ctx.r(self.local_conv.run(x.permute(0, 3, 1, 2), ctx)).permute(0, 2, 3, 1)
        return ctx.r(x + self.mlp.run(x, ctx))


class _Stage(nn.Module):
    pass


class TinyViTReference(nn.Module):
    def __init__(self, cfg: TinyViTConfig, emulate_bf16: bool = False, dtype: torch.dtype = torch.float32):
        super().__init__()
        self.cfg = cfg
        self.ctx = _Ctx()
        self.ctx.emu = emulate_bf16
        self.dt = dtype
        C = cfg.embed_dims
        self.patch_embed = PatchEmbed(C[0])
        for i in range(4):
            st = _Stage()
            if i == 0:
                st.blocks = nn.ModuleList([MBConv(C[0]) for _ in range(cfg.depths[0])])
            else:
                st.downsample = PatchMerging(C[i - 1], C[i], cfg.merge_strides[i - 1])
                st.blocks = nn.ModuleList([TinyVitBlock(C[i], cfg.num_heads[i], cfg.window_sizes[i]) for _ in range(cfg.depths[i])])
            setattr(self, f"stages_{i}", st)
        self.eval()

    def load_weights(self, w: Dict[str, np.ndarray]) -> "TinyViTReference":
        sd = {k: torch.from_numpy(np.asarray(v)) for k, v in w.items()}
        missing, unexpected = self.load_state_dict(sd, strict=False)
        assert not unexpected, unexpected
        assert all(k.endswith("num_batches_tracked") for k in missing), missing
        return self

    # ---- stage-wise entry points (NCHW in, NCHW out) -------------------------------------------------
    @torch.no_grad()
    def stem(self, x: torch.Tensor) -> torch.Tensor:
        return self.patch_embed.run(x.to(self.dt), self.ctx)

    @torch.no_grad()
    def stage(self, i: int, x: torch.Tensor) -> torch.Tensor:
        x = x.to(self.dt)
        st = getattr(self, f"stages_{i}")
        if i == 0:
            for b in st.blocks:
                x = b.run(x, self.ctx)
            return x
        x = st.downsample.run(x, self.ctx).permute(0, 2, 3, 1)
        for b in st.blocks:
            x = b.run(x, self.ctx)
        return x.permute(0, 3, 1, 2).contiguous()

    @torch.no_grad()
    def forward(self, x: torch.Tensor) -> List[torch.Tensor]:
        out = []
        x = self.stem(x)
        for i in range(4):
            x = self.stage(i, x)
            out.append(x)
        return out

    @torch.no_grad()
    def memory(self, x: torch.Tensor) -> torch.Tensor:
        """x [B,F,3,H,W] -> mean of the stage-3 map [B,F,C3] (model.py:124)."""
        B, Fr = x.shape[:2]
        return self.forward(x.reshape(B * Fr, *x.shape[2:]))[-1].mean(dim=[2, 3]).view(B, Fr, -1)


def make_frames(n: int, size: int, seed: int) -> torch.Tensor:
    """Normalised-looking random frames [n, 3, size, size] (ImageNet mean/std applied to uniform pixels)."""
    g = torch.Generator().manual_seed(seed)
    px = torch.rand(n, 3, size, size, generator=g)
    mean = torch.tensor([0.485, 0.456, 0.406]).view(1, 3, 1, 1)
    std = torch.tensor([0.229, 0.224, 0.225]).view(1, 3, 1, 1)
    return (px - mean) / std


def row_error(got: torch.Tensor, want: torch.Tensor, channel_dim: int = 1):
    """(max over rows of max|d| / row RMS, mean|d| / mean row RMS); a row = the channel vector of one pixel / frame."""
    got, want = got.double(), want.double()
    if got.dim() == 4:
        got, want = got.movedim(channel_dim, -1), want.movedim(channel_dim, -1)
    d = (got - want).abs().reshape(-1, got.shape[-1])
    rms = want.reshape(-1, want.shape[-1]).pow(2).mean(-1).sqrt().clamp_min(1e-6)
    return float((d.max(-1).values / rms).max()), float(d.mean() / rms.mean())
