"""``_WindowStream``: what CaptionStream (gitcap.model) and StudentCaptionStream (gitcap.student) share: the one-live-stream token,
the schedule and the gate in front of ``push``, and the buffers and truncation of a greedy caption."""
from __future__ import annotations

import torch

from . import _lib
from .framegate import gated_frames

STOP_NEVER, STOP_ALL_SEP = 0, 1      # the `stop` argument of the greedy entry points (include/gitcap.h)


class _WindowStream:
    """A subclass gives ``_reset_lib()`` (empty the library's window), ``_clear()`` (forget what it keeps of the frames pushed so
    far) and ``_push(frames, to_cpu)`` (encode the frames; -> the caption when one is due, else None)."""

    def __init__(self, model, sched, max_len, mode, gate, logprobs, top_logprobs=0):
        self._m, self._sched, self._gate = model, sched, gate
        self._max_len, self._mode = max_len, mode
        self._want_lp = logprobs
        self._top_k = int(top_logprobs)
        self.last_logprobs = None        # logprobs=True: fp32 [B, steps] of the caption the last push returned (on the CPU when the frames were)
        # top_logprobs=k: the k best tokens per step of that caption and their log-probabilities, [B, steps, k] each
        self.last_top_ids = self.last_top_logprobs = None
        self._token = object()
        model._window_owner = self._token            # the handle has one window: this stream owns it until the next one is opened
        self._reset_lib()

    def _check_live(self):
        if self._m._window_owner is not self._token:
            raise _lib.GitcapError(f"this {type(self).__name__} was invalidated (another caption_stream() was opened, or the model was moved)")

    def reset(self):
        """Empty the window: the next caption needs a window of new frames."""
        self._check_live()
        self._reset_lib()
        self._sched.reset()
        self._clear()
        if self._gate is not None:
            self._gate.reset()

    def push(self, frames: torch.Tensor):
        """Append one frame per clip or n of them ([B,n,...]), on the CPU or the device -> None, or the caption of the window when
        one is due (the class says which frames it takes and what a caption is); on the CPU when the frames were.  A gated stream
        takes uint8 camera frames only, [B,H,W,3] or [B,n,H,W,3]; the window and `hop` count the frames the gate admits, and a
        push with none admitted returns None."""
        self._check_live()
        if self._gate is None:
            return self._push(frames, frames.device.type == "cpu")
        admitted = gated_frames(self._gate, frames, self._sched, self._m._dev)
        return None if admitted is None else self._push(admitted, frames.device.type == "cpu")

    def _greedy_buffers(self, B):
        """-> (ids int64 [B, 1+max_len], steps int32 [1], log-probs fp32 [B, max_len] or None) for one greedy window call."""
        dev = self._m._dev
        ids = torch.empty((B, self._max_len + 1), dtype=torch.int64, device=dev)
        steps = torch.zeros((1,), dtype=torch.int32, device=dev)
        lp = torch.empty((B, self._max_len), dtype=torch.float32, device=dev) if self._want_lp else None
        return ids, steps, lp

    def _topk_buffers(self, B):
        """-> (top_ids int64, top_logprobs fp32) [B, max_len, k] for one greedy window call, or None"""
        if not self._top_k:
            return None
        dev = self._m._dev
        return (torch.empty((B, self._max_len, self._top_k), dtype=torch.int64, device=dev),
                torch.empty((B, self._max_len, self._top_k), dtype=torch.float32, device=dev))

    def _finish_greedy(self, ids, steps, lp, to_cpu, tk=None):
        """What the call left in the buffers -> the caption as greedy_decode returns it; keeps its log-probs in last_logprobs and
        its alternatives (tk = _topk_buffers') in last_top_ids / last_top_logprobs."""
        if self._mode == STOP_ALL_SEP:
            ids = ids[:, :1 + int(steps.item())]
        if tk is not None:
            self.last_top_ids, self.last_top_logprobs = ((t[:, :ids.shape[1] - 1].cpu() if to_cpu else t[:, :ids.shape[1] - 1]) for t in tk)
        if lp is not None:
            lp = lp[:, :ids.shape[1] - 1]
            self.last_logprobs = lp.cpu() if to_cpu else lp
        return ids.cpu() if to_cpu else ids
