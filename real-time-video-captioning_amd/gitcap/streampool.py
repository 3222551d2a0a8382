"""Stream pools: several live cameras on one model (StudentCaptioner.stream_pool -> ``StudentStreamPool``, include/gitcap.h:
gitcap_student_pool_*; GitCaptioner.stream_pool -> ``TeacherStreamPool``, gitcap_pool_*).  Every camera (stream) has a window of
frames of its own, at its own fill level and ring position; a push takes frames for any streams in any mix, encodes them once,
packed, and the streams that are due are captioned as one ragged batch.  ``_StreamPool`` holds what the two share -- ownership
token, schedule, chunks of max_batch, the cut behind a row's own first SEP, the ``last_*`` dicts; the subclasses differ in their
library calls only."""
from __future__ import annotations

import ctypes

import torch

from . import _lib
from ._stream import STOP_ALL_SEP
from .window import PoolSchedule


def cut_at_sep(row, sep_id: int) -> int:
    """Generated tokens of one caption row (CLS first) up to and including its own first SEP; all of them if it has none."""
    hits = (row[1:] == sep_id).nonzero()
    return int(hits[0]) + 1 if hits.numel() else row.shape[0] - 1


class _StreamPool:
    """``push(frames, streams)`` -> ``{stream: ids}`` for every stream that became due, ``caption(streams)`` for a caption now.  A
    stream's caption is bit for bit ``greedy_decode`` on a list holding that stream's last (up to `window`) frames, cut behind the
    row's OWN first SEP when the stop rule is all_sep: it does not depend on which other streams were captioned with it.  After a
    caption ``last_logprobs[stream]`` (logprobs=True), ``last_top_ids[stream]`` / ``last_top_logprobs[stream]`` (top_logprobs=k)
    and ``last_frames[stream]`` (the frames it saw) hold that caption's, cut the same way.
    Scene-change gates are not part of the pool: a caller puts one FrameGate per camera in front of ``push`` and pushes the frames
    it admits; one launch for all the gates' decisions is left to a later change.  Nor does a pool carry drafts.
    A subclass supplies ``_WHAT`` (the name of the window size in messages) and the library's side: _reset_lib, _prepare, _push_lib,
    _drop_lib, _counts_lib, _caption_lib."""

    _WHAT = "window"

    def __init__(self, model, streams, window, hop, max_len, mode, logprobs, top_logprobs, min_frames):
        self._m = model
        self._sched = PoolSchedule(streams, window, hop, min_frames)
        self._max_len, self._mode = int(max_len), mode
        self._want_lp, self._top_k = bool(logprobs), int(top_logprobs)
        self.last_logprobs, self.last_top_ids, self.last_top_logprobs, self.last_frames = {}, {}, {}, {}
        self._token = object()
        model._pool_owner = self._token             # the handle has one pool: this object owns it until the next one is opened
        self._reset_lib()

    def _check_live(self):
        if self._m._pool_owner is not self._token:
            raise _lib.GitcapError(f"this {type(self).__name__} was invalidated (another stream_pool() was opened, the model was moved or its weights were loaded again)")

    def _last_dicts(self):
        return (self.last_logprobs, self.last_top_ids, self.last_top_logprobs, self.last_frames)

    def _buffers(self, B):
        """The outputs of one greedy pool call over B rows -> (ids [B, 1+max_len], log-probs or None, (top ids, top log-probs) or None)"""
        dev, L = self._m._dev, self._max_len
        out = torch.empty((B, L + 1), dtype=torch.int64, device=dev)
        lp = torch.empty((B, L), dtype=torch.float32, device=dev) if self._want_lp else None
        tk = None
        if self._top_k:
            tk = (torch.empty((B, L, self._top_k), dtype=torch.int64, device=dev),
                  torch.empty((B, L, self._top_k), dtype=torch.float32, device=dev))
        return out, lp, tk

    # ------------------------------------------------------------------ frames in, captions out
    def push(self, frames: torch.Tensor, streams) -> dict:
        """``frames``: n frames (what the pool's model takes: see its stream_pool), on the CPU or the device; ``streams``: n ints,
        frame i belongs to stream streams[i] and is newer than that stream's earlier frames, this push's included (at most `window`
        per stream and push, at most max_batch * `window` frames per push).  The frames are encoded once, in one packed pass.
        -> {stream: ids} for every stream that is due (possibly empty); ids int64 [1 + steps] with CLS first, on the CPU when the
        frames were."""
        self._check_live()
        ids = self._sched.check(streams)
        if frames.shape[0] != len(ids):
            raise ValueError(f"{frames.shape[0]} frames for {len(ids)} stream ids")
        cap = self._m.max_batch * self._sched.window
        if len(ids) > cap:
            raise ValueError(f"a push takes at most max_batch * {self._WHAT} = {cap} frames, got {len(ids)}")
        self._push_lib(self._prepare(frames), ids)
        return self._caption(self._sched.push(ids), frames.device.type == "cpu")

    def caption(self, streams, to_cpu: bool = False) -> dict:
        """Caption these streams now, whatever the schedule says -> {stream: ids}.  Every one of them must hold a frame."""
        self._check_live()
        ids = [int(s) for s in streams]
        if len(set(ids)) != len(ids):
            raise ValueError("a stream is named twice")
        return self._caption(ids, to_cpu)

    def _caption(self, due, to_cpu: bool) -> dict:
        out = {}
        B = self._chunk_rows()
        sep = self._m.cfg.sep_token_id
        for c0 in range(0, len(due), B):
            chunk = due[c0:c0 + B]
            ids, lp, tk, seen = self._caption_lib(chunk)
            if to_cpu:
                ids = tuple(t.cpu() for t in ids) if isinstance(ids, tuple) else ids.cpu()       # (a tuple: a search's predictions and scores)
                lp, tk = None if lp is None else lp.cpu(), None if tk is None else (tk[0].cpu(), tk[1].cpu())
            self._deliver(out, chunk, ids, lp, tk, seen, to_cpu, sep)
            self._sched.captioned(chunk)
        return out

    def _chunk_rows(self) -> int:
        """Streams captioned per library call."""
        return self._m.max_batch

    def _deliver(self, out, chunk, ids, lp, tk, seen, to_cpu, sep):
        """One chunk's rows into `out` and the last_* dicts, each cut behind its own first SEP under all_sep."""
        host = ids if to_cpu or self._mode != STOP_ALL_SEP else ids.cpu()
        for r, s in enumerate(chunk):
            n = cut_at_sep(host[r], sep) if self._mode == STOP_ALL_SEP else self._max_len
            out[s] = ids[r, :1 + n]
            self.last_frames[s] = int(seen[r])
            if lp is not None:
                self.last_logprobs[s] = lp[r, :n]
            if tk is not None:
                self.last_top_ids[s], self.last_top_logprobs[s] = tk[0][r, :n], tk[1][r, :n]

    def drop(self, stream: int):
        """Empty one stream (a camera that reconnected); the others keep their frames."""
        self._check_live()
        s = int(stream)
        if not 0 <= s < self._sched.streams:
            raise ValueError(f"stream {s} outside 0..{self._sched.streams - 1}")
        self._drop_lib(s)
        self._sched.drop(s)
        for d in self._last_dicts():
            d.pop(s, None)

    def counts(self) -> list:
        """Frames held per stream, 0..`window` (the library's *_pool_counts)."""
        self._check_live()
        return self._counts_lib()


class StudentStreamPool(_StreamPool):
    """The pool of StudentCaptioner.stream_pool: windows of ``mem_tokens`` frames.  ``constraints``
    (stream_pool's constraint arguments, or None): one set of rules for every stream, attached again for every pool call.
    ``beams`` = None (greedy) or k: a caption is then the best beam [max_len] of gitcap_student_pool_beam_search (CLS first, not
    cut), max_batch // k streams per call; with ``search`` (a gitcap.student._StudentSearch) it is rank 0 of the search that ends
    hypotheses at SEP, and ``last_scores[stream]`` [n], ``last_predictions[stream]`` [n, max_len] and ``last_lengths[stream]`` [n]
    hold all ranks.  A prompt of a pool with beams takes at most max_len - 1 tokens.
    ``set_prompt(stream, ids)``: a standing text prefix per camera (include/gitcap.h: gitcap_student_attach_prompt); a pool call
    attaches the ragged table of the cameras it captions, a camera without one being the row of CLS alone, and
    ``last_prompt_lengths[stream]`` holds the prompt tokens (CLS included) of that camera's latest caption."""

    _WHAT = "mem_tokens"

    def __init__(self, model, streams, hop, max_len, mode, logprobs, top_logprobs, min_frames, constraints=None, beams=None, search=None):
        self._co, self._beams, self._se = constraints, beams, search
        self._plimit = (max_len, "max_len") if beams is None else (max_len - 1, "max_len - 1")
        if search is not None:
            self.last_scores, self.last_predictions, self.last_lengths = {}, {}, {}
        self._prompts = {}                  # stream -> its prompt, int64 1-D on the CPU, CLS first
        self.last_prompt_lengths = {}
        super().__init__(model, streams, model.cfg.mem_tokens, hop, max_len, mode, logprobs, top_logprobs, min_frames)

    def _last_dicts(self):
        own = (self.last_scores, self.last_predictions, self.last_lengths) if self._se is not None else ()
        return super()._last_dicts() + (self.last_prompt_lengths,) + own

    def _chunk_rows(self) -> int:
        return self._m.max_batch // (self._beams or 1)

    def set_prompt(self, stream: int, ids):
        """The prompt of one camera from its next caption on: ``ids`` 1-D token ids (CLS is prepended where missing; at most max_len
        tokens with it), or None for no prompt.  It stays until replaced; ``drop(stream)`` does not remove it."""
        self._check_live()
        s = int(stream)
        if not 0 <= s < self._sched.streams:
            raise ValueError(f"stream {s} outside 0..{self._sched.streams - 1}")
        if ids is None:
            self._prompts.pop(s, None)
            return
        row = torch.as_tensor(ids)
        if row.dim() != 1:
            raise ValueError(f"a camera's prompt is 1-D token ids, got {tuple(row.shape)}")
        pr = self._m._prompt([row], None, 1, *self._plimit)          # the shared normaliser: CLS, the length limit
        self._prompts[s] = pr.ids[0].cpu()

    def _chunk_prompt(self, ids):
        """The ragged prompt table of one pool call over streams `ids`, or None when none of them has a prompt"""
        if not any(s in self._prompts for s in ids):
            return None
        cls = torch.tensor([self._m.cls_token_id], dtype=torch.int64)
        return self._m._prompt([self._prompts.get(s, cls) for s in ids], None, len(ids), *self._plimit)

    def _deliver(self, out, chunk, ids, lp, tk, seen, to_cpu, sep):
        """The cut behind a row's own first SEP looks at what the model emitted: a SEP inside a camera's prompt does not end its row."""
        if self._beams is not None:         # beam captions are whole rows: the best beam, or rank 0 of (predictions, scores, lengths)
            for r, s in enumerate(chunk):
                self.last_frames[s] = int(seen[r])
                if self._se is None:
                    out[s] = ids[r]
                else:
                    out[s], self.last_predictions[s], self.last_scores[s], self.last_lengths[s] = ids[0][r, 0], ids[0][r], ids[1][r], ids[2][r]
            return
        if self._mode != STOP_ALL_SEP or all(self.last_prompt_lengths.get(s, 1) == 1 for s in chunk):
            return super()._deliver(out, chunk, ids, lp, tk, seen, to_cpu, sep)
        host = ids.cpu()
        for r, s in enumerate(chunk):
            p = self.last_prompt_lengths[s]
            n = p - 1 + cut_at_sep(host[r, p - 1:], sep)
            out[s] = ids[r, :1 + n]
            self.last_frames[s] = int(seen[r])
            if lp is not None:
                self.last_logprobs[s] = lp[r, :n]
            if tk is not None:
                self.last_top_ids[s], self.last_top_logprobs[s] = tk[0][r, :n], tk[1][r, :n]

    def _reset_lib(self):
        with torch.cuda.device(self._m._dev):
            self._m._call("gitcap_student_pool_reset", self._sched.streams)

    def _push_lib(self, mem, ids):
        m = self._m
        with torch.cuda.device(m._dev):
            m._call("gitcap_student_pool_push", _lib.ptr(mem), (ctypes.c_int32 * len(ids))(*ids), len(ids), m._stream())

    def _drop_lib(self, s):
        self._m._call("gitcap_student_pool_drop", s)

    def _counts_lib(self):
        out = (ctypes.c_int32 * self._sched.streams)()
        self._m._call("gitcap_student_pool_counts", out)
        return list(out)

    def _caption_lib(self, ids):
        """One gitcap_student_pool_greedy on streams `ids` (at most max_batch) -> (ids [B, 1+max_len], log-probs or None, (top ids,
        top log-probs) or None, frames seen per row), on the device."""
        m, B = self._m, len(ids)
        if self._beams is not None:
            return self._beam_lib(ids)
        out, lp, tk = self._buffers(B)
        seen = (ctypes.c_int32 * B)()
        with torch.cuda.device(m._dev):
            m._attach_logprobs(lp, tk)
            if self._co is not None:
                self._co.attach(m)
            pr = self._chunk_prompt(ids)
            if pr is not None:
                pr.attach(m)
            m._call("gitcap_student_pool_greedy", (ctypes.c_int32 * B)(*ids), B, self._max_len, self._mode, _lib.ptr(out), None, seen, m._stream())
        for r, s in enumerate(ids):
            self.last_prompt_lengths[s] = 1 if pr is None else pr.host_lengths[r]
        return out, lp, tk, list(seen)

    def _beam_lib(self, ids):
        """One gitcap_student_pool_beam_search on streams `ids` (at most max_batch // beams) -> (the best beams [B, max_len], or the
        search's (predictions [B, n, max_len], scores [B, n], lengths [B, n]); None; None; frames seen per row), on the device."""
        m, B = self._m, len(ids)
        sid = (ctypes.c_int32 * B)(*ids)
        call = lambda ptr: m._call("gitcap_student_pool_beam_search", sid, B, self._beams, self._max_len, ptr, m._stream())
        with torch.cuda.device(m._dev):
            if self._co is not None:
                self._co.attach(m)
            pr = self._chunk_prompt(ids)
            if pr is not None:
                pr.attach(m)
            if self._se is not None:
                res = self._se.run(m, B, self._max_len, call)
                out = (res["predictions"], res["scores"], res["lengths"])
            else:
                out = torch.empty((B, self._max_len), dtype=torch.int64, device=m._dev)
                call(_lib.ptr(out))
        held = self._counts_lib()
        for r, s in enumerate(ids):
            self.last_prompt_lengths[s] = 1 if pr is None else pr.host_lengths[r]
        return out, None, None, [held[s] for s in ids]

    def _prepare(self, frames: torch.Tensor) -> torch.Tensor:
        """uint8 [n,H,W,3] / fp32 [n,3,S,S] frames, or memory tokens [n,d_model] -> memory tokens [n,d_model] fp32 on the device."""
        m = self._m
        if frames.dtype != torch.uint8 and frames.dim() == 2:
            if frames.shape[1] != m.cfg.d_model:
                raise ValueError(f"expected memory tokens [n,{m.cfg.d_model}], got {tuple(frames.shape)}")
            return frames.to(device=m._dev, dtype=torch.float32).contiguous()
        if frames.dim() != 4:
            raise ValueError(f"expected frames [n,H,W,3] uint8, [n,3,S,S] fp32 or tokens [n,d_model], got {tuple(frames.shape)}")
        if not m._native():
            raise _lib.GitcapError("stream_pool needs the native TinyViT encoder (image_encoder='native'): frames are "
                                   "encoded one at a time on the device")
        return m._encode_packed(frames).contiguous()


class TeacherStreamPool(_StreamPool):
    """The pool of GitCaptioner.stream_pool (include/gitcap.h: gitcap_pool_*): windows of ``frames`` frames over a ring of the
    encoder's fp32 ln_post rows, so a pushed frame runs the CLIP-ViT once and a caption re-runs only the temporal add, the decoder's
    image prefix and the token loop.  ``opts`` = (prompt, constraints) as _CallOptions takes them, one set for every stream, attached
    again for every pool call.  ``beam`` = None (greedy) or (beam_size, length_penalty, per_node_beam_size): a caption is then the
    search's best hypothesis [max_len] (CLS first, EOS padded, not cut) and ``last_scores[stream]`` its score; log-probabilities and
    alternatives belong to the greedy pool.
    A failed statistics exchange (GitcapExchangeTimeout, raised once) leaves the ring's rows undefined: the library empties every
    stream, and so does the pool -- push the cameras' frames again."""

    _WHAT = "frames"

    def __init__(self, model, streams, window, hop, max_len, mode, logprobs, top_logprobs, min_frames, opts=(None, None), beam=None):
        self._opts, self._beam = opts, beam
        if beam is not None:
            self.last_scores = {}
        super().__init__(model, streams, window, hop, max_len, mode, logprobs, top_logprobs, min_frames)

    def _last_dicts(self):
        return super()._last_dicts() + ((self.last_scores,) if self._beam is not None else ())

    def _emptied(self):
        """The library emptied every stream (a failed exchange): the schedule and the last_* dicts follow."""
        self._sched.reset()
        for d in self._last_dicts():
            d.clear()

    def _reset_lib(self):
        with torch.cuda.device(self._m._dev):
            self._m._call("gitcap_pool_reset", self._sched.streams, self._sched.window)

    def _prepare(self, frames: torch.Tensor):
        """uint8 camera frames [n,H,W,3] or transformed fp32 frames [n,3,S,S], host or device -> (device frames, raw)"""
        m, S = self._m, self._m.cfg.image_size
        raw = frames.dtype == torch.uint8
        if frames.dim() != 4 or (frames.shape[3] != 3 or min(frames.shape[1:3]) < 1 if raw else tuple(frames.shape[1:]) != (3, S, S)):
            raise ValueError(f"expected frames [n,H,W,3] uint8 or [n,3,{S},{S}] fp32, got {frames.dtype} {tuple(frames.shape)}")
        return m._to_device(frames), raw

    def _push_lib(self, prepared, ids):
        m = self._m
        fr, raw = prepared
        sid = (ctypes.c_int32 * len(ids))(*ids)
        m._drain()
        try:
            with torch.cuda.device(m._dev):
                if raw:
                    m._call("gitcap_pool_push_raw", _lib.ptr(fr), sid, len(ids), fr.shape[1], fr.shape[2], m._stream())
                else:
                    m._call("gitcap_pool_push", _lib.ptr(fr), sid, len(ids), m._stream())
        except _lib.GitcapExchangeTimeout:
            self._emptied()
            raise

    def _drop_lib(self, s):
        self._m._call("gitcap_pool_drop", s)

    def _counts_lib(self):
        out = (ctypes.c_int32 * self._sched.streams)()
        self._m._call("gitcap_pool_counts", out)
        return list(out)

    def _caption_lib(self, ids):
        """One gitcap_pool_greedy (or _beam_search) on streams `ids` (at most max_batch) -> (ids [B, 1+max_len] or the search's
        (predictions [B, max_len], scores [B]), log-probs or None, (top ids, top log-probs) or None, frames seen per row)."""
        from .model import _CallOptions
        m, B = self._m, len(ids)
        sid = (ctypes.c_int32 * B)(*ids)
        prompt, cons = self._opts
        opts = _CallOptions(m, None if prompt is None else prompt.rows(0, B), cons)
        m._drain()
        try:
            with torch.cuda.device(m._dev):
                if self._beam is None:
                    out, lp, tk = self._buffers(B)
                    seen = (ctypes.c_int32 * B)()
                    opts.attach(lp, tk)
                    m._call("gitcap_pool_greedy", sid, B, self._max_len, self._mode, _lib.ptr(out), None, seen, m._stream())
                    seen = list(seen)
                else:
                    k, length_penalty, per_node = self._beam
                    own, decoded, scores = opts.search_outputs(B, self._max_len)
                    lp = tk = None
                    opts.attach()
                    m._call("gitcap_pool_beam_search", sid, B, k, self._max_len, ctypes.c_float(length_penalty), per_node, _lib.ptr(own[0]),
                            _lib.ptr(own[1]), m._stream())
                    out = (decoded, scores)
                    held = self._counts_lib()
                    seen = [held[s] for s in ids]
        except _lib.GitcapExchangeTimeout:
            self._emptied()
            raise
        m._last_memory = None
        return out, lp, tk, seen

    def _caption(self, due, to_cpu: bool) -> dict:
        out = super()._caption(due, to_cpu)
        if to_cpu and due:
            self._m.poll_errors()           # CPU results are vouched for, as caption_stream's
        return out

    def _deliver(self, out, chunk, ids, lp, tk, seen, to_cpu, sep):
        if self._beam is None:
            return super()._deliver(out, chunk, ids, lp, tk, seen, to_cpu, sep)
        decoded, scores = ids
        for r, s in enumerate(chunk):
            out[s], self.last_scores[s], self.last_frames[s] = decoded[r], scores[r], int(seen[r])
