"""``TinyViTEncoder``: the student captioner's TinyViT image encoder (timm ``TinyVit``, ``features_only=True``,
the reference's src/models/model.py:35-47, :108-126) on the HIP kernels of csrc/tinyvit.hip through the
``gitcap_tinyvit_*`` entry points (include/gitcap.h).

``forward(x [N,3,H,W])`` returns the four feature maps (fp32 NCHW, as the reference's ``image_enc_fmaps``);
``memory(x [B,F,3,H,W])`` returns the mean of the stage-3 map, ``[B,F,C3]`` fp32 (model.py:124), without writing the
feature maps.  Both also take uint8 BGR camera frames (``[N,H,W,3]`` / ``[B,F,H,W,3]``): the reference's frame transform
then runs inside the first stem convolution's gather (``gitcap_tinyvit_encode_raw``), bitwise equal to
``gitcap.preprocess.preprocess_frames`` followed by the fp32 call.  Everything runs on the caller's current stream with
no host synchronisation.  There is no CPU path."""
from __future__ import annotations

import ctypes
from dataclasses import asdict
from typing import Dict, Mapping, Optional

import numpy as np
import torch

from . import _lib
from ._handle import _NativeModule
from .tinyvit_config import (CTinyViTConfig, TinyViTConfig, canonical_key, check_tinyvit_shapes, fold_convnorm,  # noqa: F401
                             folded_tensors, normalise_keys, tinyvit_config, tinyvit_shapes, tinyvit_synthetic_weights,
                             tinyvit_tiny)


def _rebuild_tinyvit(cfg_dict, weights, kwargs):
    cfg_dict = dict(cfg_dict)
    for k in ("embed_dims", "depths", "num_heads", "window_sizes", "merge_strides"):
        cfg_dict[k] = tuple(cfg_dict[k])
    return TinyViTEncoder(TinyViTConfig(**cfg_dict), weights=weights, **kwargs)


class TinyViTEncoder(_NativeModule):
    _PREFIX, _FINALIZE = "gitcap_tinyvit", "gitcap_tinyvit_finalize"

    def __init__(self, cfg: TinyViTConfig, weights: Optional[Mapping[str, object]] = None,
                 device: str | torch.device = "cuda:0", max_frames: int = 96):
        super().__init__()
        cfg.validate()
        self.cfg = cfg
        self.max_frames = int(max_frames)
        self._dev = torch.device(device)
        self._handle = None
        self._weights: Optional[Dict[str, np.ndarray]] = None
        self._lib = _lib.load()
        self._open()
        if weights is not None:
            self.load_state_dict(weights)

    # ------------------------------------------------------------------ handle management
    def _cconfig(self):
        return CTinyViTConfig.from_config(self.cfg, self.max_frames)

    @property
    def device(self) -> torch.device:
        return self._dev

    @property
    def out_dim(self) -> int:
        return self.cfg.embed_dims[3]

    def cpu(self):
        raise _lib.GitcapError("gitcap has no CPU path; .cpu() refused")

    # ------------------------------------------------------------------ weights
    @property
    def loaded(self) -> bool:
        return self._weights is not None

    def load_state_dict(self, state_dict, strict: bool = True):
        """Takes the keys with the prefix ``image_encoder.model.``, ``model.`` or none, and ``stages_i`` or ``stages.i``;
        ``num_batches_tracked`` and ``attention_bias_idxs`` are ignored (the index table is rebuilt).  Every key of
        ``tinyvit_shapes`` must be present.  ``state_dict()`` returns them as loaded: canonical keys (``stages_i`` form, no
        prefix), BatchNorms unfolded."""
        state = normalise_keys(state_dict)
        w = {}
        for name in tinyvit_shapes(self.cfg):
            if name not in state:
                raise KeyError(f"missing TinyViT weight {name}")
            w[name] = self._as_f32(state[name])
        if strict:
            extra = sorted(set(state) - set(w))
            if extra:
                raise KeyError(f"unexpected TinyViT keys: {extra[:5]}")
        check_tinyvit_shapes(self.cfg, w)
        self._upload(w)
        self._weights = w
        return self

    def _upload(self, w):
        self._load_tensors(folded_tensors(self.cfg, w).items())

    def __reduce__(self):
        return _rebuild_tinyvit, (asdict(self.cfg), self._weights, dict(device=str(self._dev), max_frames=self.max_frames))

    # ------------------------------------------------------------------ encode
    def _frames(self, x: torch.Tensor) -> torch.Tensor:
        """[N,3,S,S] transformed frames, or uint8 BGR camera frames [N,H,W,3] (OpenCV layout, the reference's
        real_time_inference.py:39; the dtype decides, as in GitCaptioner._check_frames) -> contiguous device tensor."""
        s = self.cfg.img_size
        raw = x.dtype == torch.uint8
        if raw:
            if x.dim() != 4 or x.shape[3] != 3 or min(x.shape[1], x.shape[2]) < 1:
                raise ValueError(f"expected uint8 frames [N,H,W,3], got {tuple(x.shape)}")
        elif x.dim() != 4 or x.shape[1] != 3 or x.shape[2] != s or x.shape[3] != s:
            raise ValueError(f"expected frames [N,3,{s},{s}], got {tuple(x.shape)}")
        if x.shape[0] < 1 or x.shape[0] > self.max_frames:
            raise ValueError(f"{x.shape[0]} frames outside 1..max_frames={self.max_frames}")
        return x.to(device=self._dev, dtype=torch.uint8 if raw else torch.float32).contiguous()

    def _clips(self, x: torch.Tensor):
        """[B,F,3,S,S], or uint8 [B,F,H,W,3] ([F,H,W,3] = one clip) -> (frames [B*F,...], B, F)."""
        if x.dtype == torch.uint8 and x.dim() == 4:
            x = x.unsqueeze(0)
        if x.dim() != 5:
            raise ValueError(f"expected frames [B,F,3,H,W] or uint8 [B,F,H,W,3], got {tuple(x.shape)}")
        B, F = x.shape[:2]
        return self._frames(x.reshape(B * F, *x.shape[2:])), B, F

    def _encode(self, x: torch.Tensor, want_fmaps: bool):
        n = x.shape[0]
        mem = torch.empty((n, self.out_dim), dtype=torch.float32, device=self._dev)
        fmaps = []
        arr = None
        if want_fmaps:
            for C, m in zip(self.cfg.embed_dims, self.cfg.stage_maps()):
                fmaps.append(torch.empty((n, C, m, m), dtype=torch.float32, device=self._dev))
            ptrs = (ctypes.c_void_p * 4)(*[t.data_ptr() for t in fmaps])
            arr = ctypes.cast(ptrs, ctypes.c_void_p)
        with torch.cuda.device(self._dev):
            if x.dtype == torch.uint8:       # the transform is fused with the first stem convolution's gather
                self._call("gitcap_tinyvit_encode_raw", _lib.ptr(x), n, x.shape[1], x.shape[2], _lib.ptr(mem), arr, self._stream())
            else:
                self._call("gitcap_tinyvit_encode", _lib.ptr(x), n, _lib.ptr(mem), arr, self._stream())
        return fmaps, mem

    @torch.no_grad()
    def forward(self, x: torch.Tensor):
        """x [N,3,H,W] (normalised) or uint8 camera frames [N,H,W,3] -> list of the four stage feature maps, fp32 NCHW on
        the device."""
        return self._encode(self._frames(x), True)[0]

    @torch.no_grad()
    def forward_with_memory(self, x: torch.Tensor):
        """x [B,F,3,H,W] or uint8 [B,F,H,W,3] -> (four feature maps [B*F,Ci,Hi,Wi], memory [B,F,C3]) from one encode."""
        fr, B, F = self._clips(x)
        fmaps, mem = self._encode(fr, True)
        return fmaps, mem.view(B, F, -1)

    @torch.no_grad()
    def memory(self, x: torch.Tensor) -> torch.Tensor:
        """x [B,F,3,H,W] or uint8 [B,F,H,W,3] -> mean of the stage-3 map [B,F,C3] fp32 (model.py:124); no feature maps
        are written."""
        fr, B, F = self._clips(x)
        return self._encode(fr, False)[1].view(B, F, -1)
