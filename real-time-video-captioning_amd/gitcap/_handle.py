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
