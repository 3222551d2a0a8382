"""``_NativeModule``: what GitCaptioner, StudentCaptioner and TinyViTEncoder share as owners of one libgitcap handle (the Python
mirror of HandleCore in csrc/host_util.h).  The three families of entry points differ in their prefix only
(``<prefix>_create / _destroy / _last_error / _load_tensor``), so a subclass names its ``_PREFIX`` and ``_FINALIZE`` symbol and
fills in four hooks; the handle's life cycle, the status checks, ``to()`` and the weight upload are here."""
from __future__ import annotations

import ctypes

import numpy as np
import torch
from torch import nn

from . import _lib


class _Prompt:
    """A batch of per-clip text prefixes on the device (include/gitcap.h: gitcap_attach_prompt, gitcap_student_attach_prompt): ids
    int64 [B, P] with CLS at column 0, lengths int32 [B] (valid tokens per clip, CLS included), and the host's copy of the lengths."""

    def __init__(self, ids, lengths, host_lengths):
        self.ids, self.lengths, self.host_lengths = ids, lengths, host_lengths
        self.min_len, self.max_len = min(host_lengths), max(host_lengths)

    def rows(self, r0, r1):
        return _Prompt(self.ids[r0:r1].contiguous(), self.lengths[r0:r1].contiguous(), self.host_lengths[r0:r1])

    def attach(self, model):
        """The one-shot attachment the NEXT greedy- or beam-family call consumes (a repeated call attaches again)."""
        model._call(model._PREFIX + "_attach_prompt", _lib.ptr(self.ids), self.ids.shape[1], _lib.ptr(self.lengths), self.min_len, self.max_len)


class _NativeModule(nn.Module):
    """The constructor of a subclass sets ``_lib``, ``_dev``, ``_handle = None`` and ``_weights = None``, then calls ``_open()``."""
    _PREFIX = None       # "gitcap" | "gitcap_student" | "gitcap_tinyvit"
    _FINALIZE = None     # the symbol that ends a weight upload

    # ------------------------------------------------------------------ hooks
    def _cconfig(self):
        """-> the ctypes config struct ``<prefix>_create`` takes; sets the ``max_*`` attributes it is made from."""
        raise NotImplementedError

    def _configure(self):
        """Runs on every fresh handle, before any weight is loaded."""

    def _upload(self, w):
        """``self._load_tensors((name, array), ...)`` in the order the library expects."""
        raise NotImplementedError

    def _moved(self):
        """Runs after ``to()`` has really changed the device (new handle, weights loaded again)."""

    # ------------------------------------------------------------------ prompts (GitCaptioner and StudentCaptioner: `cls_token_id`)
    def _prompt(self, prompt, prompt_lengths, B, limit, what):
        """The ``prompt=`` argument of the decoding calls -> _Prompt or None.  prompt: int64 [B, P] (every row P tokens, or
        ``prompt_lengths`` [B] valid tokens per row) or a list of B 1-D tensors (ragged).  CLS is prepended to a row that does not
        start with it (the lengths then count it).  A set-up step: the lengths are read on the host."""
        if prompt is None:
            if prompt_lengths is not None:
                raise ValueError("prompt_lengths without prompt")
            return None
        if isinstance(prompt, torch.Tensor):
            if prompt.dim() != 2:
                raise ValueError(f"prompt must be [B, P] or a list of B 1-D tensors, got {tuple(prompt.shape)}")
            lens = [prompt.shape[1]] * prompt.shape[0] if prompt_lengths is None else [int(v) for v in torch.as_tensor(prompt_lengths).tolist()]
            if len(lens) != prompt.shape[0] or any(not 0 <= n <= prompt.shape[1] for n in lens):
                raise ValueError("prompt_lengths must hold one length in [0, P] per row of prompt")
            host = prompt.detach().to("cpu", torch.int64)
            rows = [host[b, :n] for b, n in enumerate(lens)]
        else:
            if prompt_lengths is not None:
                raise ValueError("prompt_lengths goes with a [B, P] tensor; a list of rows carries its own lengths")
            rows = [torch.as_tensor(r).detach().to("cpu", torch.int64).reshape(-1) for r in prompt]
        if len(rows) != B:
            raise ValueError(f"prompt has {len(rows)} rows for a batch of {B} clips")
        cls = self.cls_token_id
        rows = [r if r.numel() and int(r[0]) == cls else torch.cat([torch.tensor([cls], dtype=torch.int64), r]) for r in rows]
        lens = [int(r.numel()) for r in rows]
        if max(lens) > limit:
            raise ValueError(f"a prompt of {max(lens)} tokens (CLS included) exceeds {what} = {limit}")
        ids = torch.full((B, max(lens)), cls, dtype=torch.int64)
        for b, r in enumerate(rows):
            ids[b, :lens[b]] = r
        return _Prompt(ids.to(self._dev), torch.tensor(lens, dtype=torch.int32).to(self._dev), lens)

    # ------------------------------------------------------------------ handle
    def _open(self):
        if self._dev.type != "cuda":
            raise _lib.GitcapError("gitcap runs on an AMD GPU only (no CPU path); got device %s" % self._dev)
        if not torch.cuda.is_available():
            raise _lib.GitcapError("no HIP device visible: gitcap has no CPU fallback")
        self._create_on(self._dev.index if self._dev.index is not None else torch.cuda.current_device())

    def _create_on(self, idx: int):
        self._dev = torch.device("cuda", idx)
        cc, h = self._cconfig(), ctypes.c_void_p()
        name = self._PREFIX + "_create"
        self._check(None, getattr(self._lib, name)(ctypes.byref(cc), idx, ctypes.byref(h)), name)
        self._handle = h
        self._configure()

    def _close(self):
        h = getattr(self, "_handle", None)           # (no attribute yet: an __init__ that raised early)
        if h:
            self._handle = None                      # first: whatever happens next, nobody destroys it twice
            getattr(self._lib, self._PREFIX + "_destroy")(h)

    def __del__(self):
        try:
            self._close()
        except Exception:
            pass

    def _check(self, handle, rc, what):
        _lib.check(self._lib, handle, rc, what, self._PREFIX + "_last_error")

    def _call(self, name, *args):
        self._check(self._handle, getattr(self._lib, name)(self._handle, *args), name)

    def _stream(self):
        return ctypes.c_void_p(torch.cuda.current_stream(self._dev).cuda_stream)

    # ------------------------------------------------------------------ nn.Module surface
    @staticmethod
    def _device_arg(args, kwargs):
        """The device a ``to(...)`` call names, or None (a call that names none, e.g. a dtype, is ignored)."""
        dev = kwargs.get("device", args[0] if args else None)
        return torch.device(dev) if isinstance(dev, (str, torch.device)) else None

    def to(self, *args, **kwargs):
        dev = self._device_arg(args, kwargs)
        if dev is not None:
            if dev.type != "cuda":
                raise _lib.GitcapError("gitcap has no CPU path; .to(%s) refused" % dev)
            idx = dev.index if dev.index is not None else torch.cuda.current_device()
            if idx != self._dev.index:
                self._close()                        # _handle is None from here: if the re-create raises, __del__ has nothing to free
                self._dev = torch.device("cuda", idx)
                self._open()
                if self._weights is not None:
                    self._upload(self._weights)
                self._moved()
        return self

    # ------------------------------------------------------------------ weights
    @staticmethod
    def _as_f32(v) -> np.ndarray:
        return np.ascontiguousarray(v.detach().cpu().float().numpy() if hasattr(v, "detach") else v, dtype=np.float32)

    def state_dict(self, *a, **k):
        return {n: torch.from_numpy(v) for n, v in (self._weights or {}).items()}

    def _load_tensors(self, items):
        with torch.cuda.device(self._dev):
            for name, arr in items:
                arr = np.ascontiguousarray(arr, dtype=np.float32)
                shape = (ctypes.c_int64 * arr.ndim)(*arr.shape)
                self._call(self._PREFIX + "_load_tensor", name.encode(), arr.ctypes.data_as(ctypes.c_void_p), shape, arr.ndim)
            self._call(self._FINALIZE)
