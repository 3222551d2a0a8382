"""TinyViT encoder configuration, checkpoint keys and weight preparation (host side, no GPU).

The student captioner's image encoder is timm's ``TinyVit`` loaded with ``features_only=True``
(the reference's src/models/model.py:35-47).  timm is not a dependency: the architecture is written from its
published description (DESIGN.md "TinyViT encoder" lists what is not verified against timm).  Kept apart from
``gitcap.tinyvit`` so that ``gitcap._lib`` can import the ctypes struct without importing the module class."""
from __future__ import annotations

import ctypes
from collections import OrderedDict
from dataclasses import dataclass
from typing import Dict, Mapping, Tuple

import numpy as np


@dataclass
class TinyViTConfig:
    img_size: int = 224
    embed_dims: Tuple[int, int, int, int] = (96, 192, 384, 576)
    depths: Tuple[int, int, int, int] = (2, 2, 6, 2)
    num_heads: Tuple[int, int, int, int] = (3, 6, 12, 18)
    window_sizes: Tuple[int, int, int, int] = (7, 7, 14, 7)
    # stride of the depthwise conv of the PatchMerging into stages 1, 2, 3 (timm's reported reductions 4/8/16/32 imply
    # (2, 2, 2); Microsoft's original TinyViT uses (2, 2, 1)) -- unverified, DESIGN.md
    merge_strides: Tuple[int, int, int] = (2, 2, 2)
    ln_eps: float = 1e-5
    bn_eps: float = 1e-5

    def stage_maps(self) -> Tuple[int, int, int, int]:
        m = self.img_size // 4
        out = [m]
        for s in self.merge_strides:
            m //= s
            out.append(m)
        return tuple(out)

    def validate(self) -> None:
        if self.img_size <= 0 or self.img_size % 4:
            raise ValueError("img_size must be a positive multiple of 4")
        if len(self.merge_strides) != 3 or any(s not in (1, 2) for s in self.merge_strides):
            raise ValueError("merge_strides: three strides, each 1 or 2")
        for i in range(4):
            if self.embed_dims[i] % 32 or self.embed_dims[i] <= 0:
                raise ValueError("embed_dims must be multiples of 32")
            if self.embed_dims[i] != 32 * self.num_heads[i]:
                raise ValueError("head_dim must be 32 (embed_dims[i] == 32 * num_heads[i])")
        m = self.img_size // 4
        for i in range(1, 4):
            if self.merge_strides[i - 1] == 2 and m % 2:
                raise ValueError("a stride-2 merge needs an even map")
            m //= self.merge_strides[i - 1]
            if not 1 <= self.window_sizes[i] <= 14 or m % self.window_sizes[i]:
                raise ValueError(f"stage {i}: map {m} is not a multiple of window {self.window_sizes[i]} (or window > 14)")


_VARIANTS = {
    "tiny_vit_5m_224": dict(embed_dims=(64, 128, 160, 320), num_heads=(2, 4, 5, 10)),
    "tiny_vit_11m_224": dict(embed_dims=(64, 128, 256, 448), num_heads=(2, 4, 8, 14)),
    "tiny_vit_21m_224": dict(embed_dims=(96, 192, 384, 576), num_heads=(3, 6, 12, 18)),
}


def tinyvit_config(name: str, merge_strides: Tuple[int, int, int] = (2, 2, 2)) -> TinyViTConfig:
    """timm model name -> config, matched by prefix (``tiny_vit_21m_224.dist_in22k_ft_in1k`` is the 21m variant)."""
    for prefix, kw in _VARIANTS.items():
        if name == prefix or name.startswith(prefix + "."):
            return TinyViTConfig(merge_strides=tuple(merge_strides), **kw)
    raise ValueError(f"unknown TinyViT variant {name!r} (known: {', '.join(_VARIANTS)})")


def tinyvit_tiny(merge_strides: Tuple[int, int, int] = (2, 2, 2)) -> TinyViTConfig:
    """Small test config whose last width (64) is student_tiny's d_model; stage 1 (8x8 map, window 4) has four windows,
    and so has stage 3 with merge_strides (2, 2, 1)."""
    return TinyViTConfig(img_size=64, embed_dims=(32, 32, 64, 64), depths=(2, 2, 2, 1), num_heads=(1, 1, 2, 2),
                         window_sizes=(4, 4, 4, 2), merge_strides=tuple(merge_strides))


def convnorm_prefixes(cfg: TinyViTConfig):
    """(prefix, cout, cin per group, k, depthwise) of every Conv2d(bias=False) + BatchNorm2d pair, in forward order."""
    C = cfg.embed_dims
    out = [("patch_embed.conv1", C[0] // 2, 3, 3, False), ("patch_embed.conv2", C[0], C[0] // 2, 3, False)]
    for i in range(4):
        c = C[i]
        if i > 0:
            out += [(f"stages_{i}.downsample.conv1", c, C[i - 1], 1, False), (f"stages_{i}.downsample.conv2", c, 1, 3, True),
                    (f"stages_{i}.downsample.conv3", c, c, 1, False)]
        for j in range(cfg.depths[i]):
            bp = f"stages_{i}.blocks.{j}."
            if i == 0:
                out += [(bp + "conv1", 4 * c, c, 1, False), (bp + "conv2", 4 * c, 1, 3, True), (bp + "conv3", c, 4 * c, 1, False)]
            else:
                out.append((bp + "local_conv", c, 1, 3, True))
    return out


def tinyvit_shapes(cfg: TinyViTConfig) -> "OrderedDict[str, tuple]":
    """Checkpoint key -> shape (timm's FeatureListNet names with the ``stages_i`` form, BatchNorm buffers without
    ``num_batches_tracked``; the non-persistent ``attention_bias_idxs`` is rebuilt, never read)."""
    s: "OrderedDict[str, tuple]" = OrderedDict()
    conv = {p: (co, ci, k) for p, co, ci, k, _ in convnorm_prefixes(cfg)}

    def convnorm(p):
        co, ci, k = conv[p]
        s[p + ".conv.weight"] = (co, ci, k, k)
        for n in ("weight", "bias", "running_mean", "running_var"):
            s[p + ".bn." + n] = (co,)

    C = cfg.embed_dims
    convnorm("patch_embed.conv1")
    convnorm("patch_embed.conv2")
    for i in range(4):
        c = C[i]
        if i > 0:
            for k in (1, 2, 3):
                convnorm(f"stages_{i}.downsample.conv{k}")
        for j in range(cfg.depths[i]):
            bp = f"stages_{i}.blocks.{j}."
            if i == 0:
                for k in (1, 2, 3):
                    convnorm(bp + f"conv{k}")
                continue
            ws = cfg.window_sizes[i]
            s[bp + "attn.norm.weight"] = (c,); s[bp + "attn.norm.bias"] = (c,)
            s[bp + "attn.qkv.weight"] = (3 * c, c); s[bp + "attn.qkv.bias"] = (3 * c,)
            s[bp + "attn.proj.weight"] = (c, c); s[bp + "attn.proj.bias"] = (c,)
            s[bp + "attn.attention_biases"] = (cfg.num_heads[i], ws * ws)
            convnorm(bp + "local_conv")
            s[bp + "mlp.norm.weight"] = (c,); s[bp + "mlp.norm.bias"] = (c,)
            s[bp + "mlp.fc1.weight"] = (4 * c, c); s[bp + "mlp.fc1.bias"] = (4 * c,)
            s[bp + "mlp.fc2.weight"] = (c, 4 * c); s[bp + "mlp.fc2.bias"] = (c,)
    return s


_PREFIXES = ("image_encoder.model.", "model.")
_IGNORED = ("num_batches_tracked", "attention_bias_idxs")


def canonical_key(key: str):
    """A checkpoint key in any accepted form -> the canonical ``stages_i`` key, or None for an ignored buffer.
    Accepted: prefix ``image_encoder.model.``, ``model.`` or none; ``stages_i.`` or ``stages.i.``."""
    for p in _PREFIXES:
        if key.startswith(p):
            key = key[len(p):]
            break
    if key.rsplit(".", 1)[-1] in _IGNORED:
        return None
    if key.startswith("stages.") and len(key) > 7 and key[7].isdigit():
        key = "stages_" + key[7:]
    return key


def normalise_keys(state: Mapping[str, object]) -> Dict[str, object]:
    out = {}
    for k, v in state.items():
        ck = canonical_key(k)
        if ck is not None:
            out[ck] = v
    return out


def fold_convnorm(w: np.ndarray, gamma: np.ndarray, beta: np.ndarray, mean: np.ndarray, var: np.ndarray, eps: float = 1e-5):
    """Conv2d(bias=False) + eval BatchNorm2d -> (weight, bias) of one Conv2d: scale = gamma / sqrt(var + eps) (fp64)."""
    scale = gamma.astype(np.float64) / np.sqrt(var.astype(np.float64) + eps)
    wf = w.astype(np.float64) * scale[:, None, None, None]
    bf = beta.astype(np.float64) - mean.astype(np.float64) * scale
    return wf.astype(np.float32), bf.astype(np.float32)


def folded_tensors(cfg: TinyViTConfig, w: Mapping[str, np.ndarray]) -> "OrderedDict[str, np.ndarray]":
    """Canonical checkpoint tensors -> the tensors gitcap_tinyvit_load_tensor takes (every ConvNorm folded into
    ``<prefix>.weight`` / ``<prefix>.bias``; the other tensors as they are)."""
    out: "OrderedDict[str, np.ndarray]" = OrderedDict()
    conv = {p for p, *_ in convnorm_prefixes(cfg)}
    for name in tinyvit_shapes(cfg):
        p = name.rsplit(".", 2)[0]
        if p in conv:
            if name.endswith(".conv.weight"):
                out[p + ".weight"], out[p + ".bias"] = fold_convnorm(
                    w[name], w[p + ".bn.weight"], w[p + ".bn.bias"], w[p + ".bn.running_mean"], w[p + ".bn.running_var"],
                    cfg.bn_eps)
            continue
        out[name] = np.ascontiguousarray(w[name], dtype=np.float32)
    return out


def check_tinyvit_shapes(cfg: TinyViTConfig, w: Mapping[str, np.ndarray]) -> None:
    for name, shape in tinyvit_shapes(cfg).items():
        if name not in w:
            raise KeyError(f"missing TinyViT weight {name}")
        if tuple(w[name].shape) != tuple(shape):
            raise ValueError(f"TinyViT weight {name}: shape {tuple(w[name].shape)} != {tuple(shape)}")


def tinyvit_synthetic_weights(cfg: TinyViTConfig, seed: int = 0) -> Dict[str, np.ndarray]:
    """Random weights in checkpoint form.  Unlike timm's init, every BatchNorm has non-trivial statistics, the conv3
    gammas of the MBConvs are non-zero (timm starts them at 0, which would hide the branch) and the attention biases
    are non-zero."""
    rng = np.random.default_rng(seed)
    w: Dict[str, np.ndarray] = {}
    for name, shape in tinyvit_shapes(cfg).items():
        leaf = name.rsplit(".", 1)[-1]
        if name.endswith(".conv.weight"):
            fan_in = int(np.prod(shape[1:]))
            v = rng.standard_normal(shape) / np.sqrt(fan_in)
        elif ".bn." in name:
            v = {"weight": rng.uniform(0.5, 1.2, shape), "bias": rng.normal(0, 0.1, shape),
                 "running_mean": rng.normal(0, 0.1, shape), "running_var": rng.uniform(0.5, 1.5, shape)}[leaf]
        elif name.endswith("attention_biases"):
            v = rng.normal(0, 0.5, shape)
        elif ".norm." in name:
            v = 1.0 + rng.normal(0, 0.1, shape) if leaf == "weight" else rng.normal(0, 0.05, shape)
        elif leaf == "weight":
            v = rng.standard_normal(shape) / np.sqrt(shape[1])
        else:
            v = rng.normal(0, 0.02, shape)
        w[name] = np.ascontiguousarray(v, dtype=np.float32)
    return w


class CTinyViTConfig(ctypes.Structure):
    """Field order of ``struct gitcap_tinyvit_config`` (include/gitcap.h)."""
    _fields_ = [("img_size", ctypes.c_int32), ("embed_dims", ctypes.c_int32 * 4), ("depths", ctypes.c_int32 * 4),
                ("num_heads", ctypes.c_int32 * 4), ("window_sizes", ctypes.c_int32 * 4), ("merge_strides", ctypes.c_int32 * 4),
                ("max_frames", ctypes.c_int32), ("ln_eps", ctypes.c_float)]

    @classmethod
    def from_config(cls, cfg: TinyViTConfig, max_frames: int) -> "CTinyViTConfig":
        a4 = ctypes.c_int32 * 4
        return cls(cfg.img_size, a4(*cfg.embed_dims), a4(*cfg.depths), a4(*cfg.num_heads), a4(*cfg.window_sizes),
                   a4(0, *cfg.merge_strides), max_frames, cfg.ln_eps)
