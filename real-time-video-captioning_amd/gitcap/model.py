"""Python host side of libgitcap: an ``nn.Module`` with the call surface the reference's
callers use, so it can stand in for the model object of farazali7/real-time-video-captioning.

Mirrored interface (reference file:line):
  * ``greedy_decode(src, max_len)``           src/models/model.py:156-187, called by
                                              src/real_time_inference.py:58, src/inference.py:51
  * ``forward_image_enc(x)``                  src/models/model.py:114-133
  * ``forward_decoder(y, memory)``            src/models/model.py:135-154
  * ``forward(x, y)``                         src/models/model.py:105-112
  * ``forward_output_logits(x, y)``           src/models/model.py:747-760 (teacher)
  * ``beam_search(src, max_len, k)``          src/models/model.py:189-317 (signature)
  * ``eval() / to() / load_state_dict()``     src/inference.py:38-40
  * picklable                                 src/real_time_inference.py:8-9 (torch.load of a whole module)

PyTorch is used for device buffers and the current HIP stream only; every FLOP of the path runs
in the hand-written gfx950 kernels behind the C ABI (include/gitcap.h).
"""
from __future__ import annotations

import ctypes
import math
import os
import weakref
from typing import Dict, Mapping, Optional

import numpy as np
import torch

from . import _lib, ragged
from .config import CGitCapConfig, GitCapConfig, git_base
from .framegate import FrameGate
from . import weights as W
from ._handle import _NativeModule, _Prompt  # noqa: F401  (_Prompt: the prompts _CallOptions carries)
from ._stream import STOP_ALL_SEP, STOP_NEVER, _WindowStream
from .streampool import TeacherStreamPool
from .window import WindowSchedule


class _Submission:
    """One gitcap_greedy_submit / gitcap_beam_search_submit (possibly several coalesced caller batches); keeps its buffers
    alive until every future attached to it has delivered its result (the frames are what a poisoned submission is re-run from)."""

    def __init__(self, ticket, frames, outs, coalesced, users=1, parts=None):
        self.ticket, self.frames, self.outs, self.coalesced, self.users = ticket, frames, outs, coalesced, users
        self.parts = parts           # host-fed submissions: the callers' CPU tensors (frames is then their list; a re-run reads them)
        self.waited = False
        self.done_ev = None          # recorded on the stream that waited: fires once the submission's last launch has finished
        self.poisoned = False        # in flight when the LayerNorm statistics exchange failed: results undefined, re-run
        self.owner = None            # the model: forgets the submission once every future has delivered

    def rows(self, r0, r1):
        """Frames of caller rows [r0, r1) (what a re-run of a poisoned submission decodes again)."""
        if self.parts is None:
            return self.frames[r0:r1]
        at = 0
        for p in self.parts:
            if at == r0 and at + p.shape[0] == r1:
                return p
            at += p.shape[0]
        return torch.cat(list(self.parts), 0)[r0:r1]

    def release(self):
        self.users -= 1
        if self.users <= 0:
            self.frames = self.parts = None
            if self.owner is not None:
                self.owner._undelivered.discard(self)


class _StagingRing:
    """Host-fed submissions (the reference's callers hold CPU tensors: src/real_time_inference.py:39-58 OpenCV frames,
    src/inference.py:45-51 a DataLoader batch): a ring of pinned host buffers + device buffers, so that the host -> device copy
    of batch i + 1 runs under the compute of batch i.  The copy is enqueued on the CALLER's current stream and the submission is
    made behind it (include/gitcap.h: gitcap_greedy_submit orders the image pass behind the work already on `stream`): the
    caller's stream carries nothing else but the waits for earlier results, so the copy starts at once, and only the image pass
    waits for it.  (A stream of the ring's own -- own_stream=True, GITCAP_COPY_STREAM=own -- is a FIFTH stream beside the
    caller's, the encoder's and the two decode streams; the runtime multiplexes streams onto four hardware queues, the copy then
    queues behind a token loop and every image pass starts late: 1 618 instead of 2 004 captions/s host-fed,
    profiles/r06_host_fed_copy_stream.txt -- the same effect as the fifth stream of round 3's two-encoder experiment.)

    Pageable sources are copied into the pinned buffer by gitcap_host_copy (up to 8 threads, sized to the CPU quota: ATen's own
    parallel copy sizes its pool to the whole machine and takes 20 ms per batch under a 16-core quota); page-locked sources
    (DataLoader(pin_memory=True), a capture ring) are copied from where they are -- asynchronously: the caller must leave such a
    buffer alone until the submission's result() (the usual contract of a non_blocking copy; the future keeps a reference).

    Depth = the library's four slots.  An entry is reused four submissions later; before its device buffer is overwritten the
    copy's stream waits for the submission that read it (its `done_ev`, or the library's own wait while it is still in flight),
    and the host waits for the entry's previous host -> device copy before touching the pinned buffer."""
    DEPTH = 4

    def __init__(self, dev, lib, own_stream=False):
        self.dev, self.lib = dev, lib
        self.stream = torch.cuda.Stream(device=dev) if own_stream else None      # None: the caller's current stream (see above)
        self.entries = [dict(pinned=None, device=None, ev=None, sub=None) for _ in range(self.DEPTH + 1)]   # [-1]: synchronous calls
        self.n = 0

    def copy_stream(self):
        return self.stream if self.stream is not None else torch.cuda.current_stream(self.dev)

    def _host_copy(self, dst, src):
        """src (CPU tensor, any memory) -> dst (a view of the pinned buffer, same shape)."""
        if src.dtype == dst.dtype and src.is_contiguous():
            nbytes = src.numel() * src.element_size()
            rc = self.lib.gitcap_host_copy(_lib.ptr(dst), _lib.ptr(src), nbytes)
            if rc != 0:
                raise _lib.GitcapError(f"gitcap_host_copy failed (status {rc})")
        else:
            dst.copy_(src)                            # strided or another dtype: ATen's copy converts

    @staticmethod
    def _grow(e, nbytes, dev):
        if e["pinned"] is None or e["pinned"].numel() < nbytes:
            cap = (nbytes + (1 << 20) - 1) >> 20 << 20
            e["pinned"] = torch.empty((cap,), dtype=torch.uint8, pin_memory=True)
            e["device"] = torch.empty((cap,), dtype=torch.uint8, device=dev)

    def stage(self, model, parts, dtype, stream=None):
        """Copy the CPU tensors `parts` (same trailing shape; concatenated along dim 0) to the device.  stream=None: the
        pipelined form (next ring entry, the ring's copy stream = the caller's current stream by default); else the synchronous
        form on that stream, in the entry of its own.
        Returns (device tensor, entry, the stream the copy was enqueued on)."""
        sync = stream is not None
        e = self.entries[-1] if sync else self.entries[self.n % self.DEPTH]
        if not sync:
            self.n += 1
        st = stream if sync else self.copy_stream()
        rows = sum(p.shape[0] for p in parts)
        shape = (rows,) + tuple(parts[0].shape[1:])
        nbytes = rows * int(np.prod(parts[0].shape[1:])) * torch.empty((), dtype=dtype).element_size()
        if e["ev"] is not None:
            e["ev"].synchronize()                     # the pinned buffer's previous host -> device copy
        prev = e["sub"]
        if prev is not None:                          # the device buffer's previous reader (an image pass)
            if prev.done_ev is not None:
                st.wait_event(prev.done_ev)
            elif not prev.poisoned and prev in model._inflight:
                try:
                    model._call("gitcap_greedy_wait", prev.ticket, ctypes.c_void_p(st.cuda_stream))
                except _lib.GitcapExchangeTimeout:    # (the device was drained when the failure was taken)
                    prev.poisoned = True
            e["sub"] = None
        self._grow(e, nbytes, self.dev)
        dview = e["device"][:nbytes].view(dtype).view(shape)
        direct = len(parts) == 1 and parts[0].is_pinned() and parts[0].dtype == dtype and parts[0].is_contiguous()
        if direct:
            hsrc = parts[0]                           # already page-locked (DataLoader(pin_memory=True), a capture ring): no staging copy
        else:
            hsrc = e["pinned"][:nbytes].view(dtype).view(shape)
            r0 = 0
            for p in parts:
                self._host_copy(hsrc[r0:r0 + p.shape[0]], p)
                r0 += p.shape[0]
        with torch.cuda.stream(st):
            dview.copy_(hsrc, non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(st)
        e["ev"] = ev
        return dview, e, st


class _Constraints:
    """Hard constraints of a decoding call on the device (include/gitcap.h: gitcap_attach_constraints): the n-gram size, the
    minimum length and the suppress list as a device int32 tensor (held until the result: a submission reads it)."""

    def __init__(self, model, n, min_length, suppress):
        self.n, self.min_length, self.suppress = n, min_length, tuple(suppress)
        self.key = (n, min_length, self.suppress)
        self._ids = torch.tensor(suppress, dtype=torch.int32, device=model._dev) if suppress else None
        self._c = _lib.CConstraints(n, min_length, None if self._ids is None else self._ids.data_ptr(), len(suppress))

    def attach(self, model):
        """The one-shot attachment the NEXT greedy- or beam-family call consumes (a repeated call attaches again)."""
        model._call("gitcap_attach_constraints", ctypes.byref(self._c))


class _CallOptions:
    """Everything one decoding call attaches (include/gitcap.h: gitcap_attach_*): prompt, constraints, per-clip frame counts,
    search options and sampling.  The attachments are one-shot: ``attach`` is made before every issue of the call, a repeat after
    a failed statistics exchange and a future's re-run included; with all parts at their defaults it attaches nothing.  A future
    holds the object until its result (the device reads the prompt, the suppress list and the n-best buffers)."""

    def __init__(self, model, prompt=None, cons=None, counts=None, num_keep_best=1, repetition_penalty=1.0, sampling=None):
        self._m, self.prompt, self.cons, self.counts = model, prompt, cons, counts
        self.num_keep_best, self.repetition_penalty = int(num_keep_best), float(repetition_penalty)
        self.sampling = sampling         # None | (temperature, top_k, top_p, seed)
        self._so = self._smp = None
        self.top_k = 0                   # greedy calls: top_logprobs=k, the k best alternatives per position (0: none)
        if sampling is not None:
            self._smp = _lib.CSamplingOptions(sampling[0], sampling[1], sampling[2], sampling[3] & (2 ** 64 - 1))

    @property
    def key(self):
        """What batches must share to coalesce: a prompted batch is alone with its key, constrained ones need equal constraints."""
        return (None if self.prompt is None else id(self.prompt), None if self.cons is None else self.cons.key, self.top_k)

    def rows(self, b0, b1):
        """The options of clips [b0, b1): a chunk of a synchronous call over more than max_batch clips."""
        n = len(self.counts) if self.counts is not None else len(self.prompt.host_lengths) if self.prompt is not None else None
        if n is None or (b0 == 0 and b1 >= n):
            return self
        part = _CallOptions(self._m, None if self.prompt is None else self.prompt.rows(b0, b1), self.cons,
                            None if self.counts is None else self.counts[b0:b1], self.num_keep_best, self.repetition_penalty, self.sampling)
        part.top_k = self.top_k
        return part

    def search_outputs(self, B, max_steps):
        """The output buffers of a search over B clips -> (own, decoded, logprobs): ``own`` = the (decoded, logprobs) pair the call
        itself writes (rank 0), decoded / logprobs = what the caller gets: the same pair, or with num_keep_best > 1 the attached
        n-best buffers [B, n, max_steps] / [B, n] (own is cut from the same two allocations: whoever holds the result keeps both alive)."""
        dev, n = self._m._dev, self.num_keep_best
        ids = torch.empty((B * (n + 1) * max_steps if n > 1 else B * max_steps,), dtype=torch.int64, device=dev)
        lps = torch.empty((B * (n + 1) if n > 1 else B,), dtype=torch.float32, device=dev)
        if n == 1:
            own = decoded, logprobs = ids.view(B, max_steps), lps
            nbest = nbest_lp = None
        else:                            # [B, n, ...] with room for the call's own [B, ...] outputs behind it
            decoded, logprobs = nbest, nbest_lp = ids[:B * n * max_steps].view(B, n, max_steps), lps[:B * n].view(B, n)
            own = (ids[B * n * max_steps:].view(B, max_steps), lps[B * n:])
        if n > 1 or self.repetition_penalty != 1.0:
            self._so = _lib.CSearchOptions(n, self.repetition_penalty, None if nbest is None else nbest.data_ptr(),
                                           None if nbest_lp is None else nbest_lp.data_ptr())
        return own, decoded, logprobs

    def topk_buffers(self, nb, max_len):
        """-> (top_ids int64, top_logprobs fp32) [nb, max_len, top_k] for one greedy call, or None without top_logprobs"""
        if not self.top_k:
            return None
        dev = self._m._dev
        return (torch.empty((nb, max_len, self.top_k), dtype=torch.int64, device=dev),
                torch.empty((nb, max_len, self.top_k), dtype=torch.float32, device=dev))

    def attach(self, lp=None, tk=None):
        """lp: the token log-probability buffer [nb, max_len] of a greedy call (one per chunk); tk: its topk_buffers()."""
        m = self._m
        if lp is not None:
            m._call("gitcap_attach_token_logprobs", _lib.ptr(lp), lp.shape[1])
        if tk is not None:
            m._call("gitcap_attach_top_logprobs", tk[0].shape[2], _lib.ptr(tk[0]), _lib.ptr(tk[1]), tk[0].shape[1])
        if self._so is not None:
            m._call("gitcap_attach_search_options", ctypes.byref(self._so))
        if self._smp is not None:
            m._call("gitcap_attach_sampling", ctypes.byref(self._smp))
        if self.prompt is not None:
            self.prompt.attach(m)
        if self.cons is not None:
            self.cons.attach(m)
        if self.counts is not None:
            m._attach_counts(self.counts)


def _lp2d(logprobs):
    """The search's scores as the reference returns them, [B, num_keep_best] (the one-hypothesis call writes [B])."""
    return logprobs[:, None] if logprobs.dim() == 1 else logprobs


class _Future:
    """Common part of the result handles: wait, vouch for the result where a host synchronisation makes that possible, and
    re-run the batch on the (by then degraded) handle if the submission was poisoned by a failed statistics exchange."""

    def _deliver(self, extract, synced, rerun):
        m, sub = self._m, self._sub
        m._wait_submission(sub)
        out = None
        if not sub.poisoned:
            out = extract()
            if synced:                         # the data is on the host (or a .item() went through): the flag is meaningful now
                try:
                    m.poll_errors()
                except _lib.GitcapExchangeTimeout:
                    m._poison_inflight()
                    sub.poisoned = True
        if sub.poisoned:
            out = rerun()
        sub.release()
        return out


class CaptionFuture(_Future):
    """Result handle of greedy_decode_async."""

    def __init__(self, model, frames, mode, max_len, out_device, opts):
        self._m, self._frames, self._mode, self._max_len, self._out_device = model, frames, mode, max_len, out_device
        self._sub, self._r0, self._r1 = None, 0, 0
        self._done = None
        self._opts = opts                        # _CallOptions: held until the result (the device reads it; a re-run attaches it again)

    def _attach(self, sub, r0, r1):
        self._sub, self._r0, self._r1 = sub, r0, r1
        self._frames = None                      # the submission holds the (concatenated) frames now

    def result(self) -> torch.Tensor:
        if self._done is not None:
            return self._done
        m = self._m
        if self._sub is None:                    # still waiting for partners to coalesce with: run now
            m._flush_pending()
        sub = self._sub

        def extract():
            ids = sub.outs[0][self._r0:self._r1]
            if self._mode == STOP_ALL_SEP:
                if sub.coalesced:                    # reference rule over THIS caller batch (model.py:184)
                    all_sep = (ids[:, 1:] == m.sep_token_id).all(dim=0)
                    nz = torch.nonzero(all_sep)
                    n = int(nz[0].item()) + 1 if nz.numel() else self._max_len
                else:
                    n = int(sub.outs[1].item())
                ids = ids[:, :1 + n]
            mv = lambda t: t.to(self._out_device) if self._out_device != t.device else t
            if self._opts.top_k:                     # (ids, top_ids, top_logprobs), as greedy_decode(top_logprobs=k)
                return (mv(ids),) + tuple(mv(t[self._r0:self._r1, :ids.shape[1] - 1]) for t in sub.outs[2:4])
            return mv(ids)

        def rerun():
            counts, rg = self._opts.counts, None
            if counts is not None:               # a ragged batch: the callers' host clips again, or the packed device frames clip by clip
                clips = sub.parts if sub.parts is not None else list(torch.split(sub.frames, counts))
                rg = (clips, counts, clips[0].dtype == torch.uint8)
            out = m._greedy_decode(None if rg is not None else sub.rows(self._r0, self._r1), self._max_len, self._mode, False, self._opts, rg)
            mv = lambda t: t.to(self._out_device) if self._out_device != t.device else t
            return tuple(mv(t) for t in out) if isinstance(out, tuple) else mv(out)

        synced = self._mode == STOP_ALL_SEP or self._out_device.type == "cpu"
        self._done = self._deliver(extract, synced, rerun)
        return self._done


class InferFuture(_Future):
    """Result handle of infer_async: ``result()`` returns the dict of ``GitCaptioner.infer``."""

    def __init__(self, model, sub, opts, search, out_device, save_logits):
        self._m, self._sub, self._opts, self._out_device, self._save = model, sub, opts, out_device, save_logits
        self._search = search                    # the search's plain arguments: beam_size, max_steps, length_penalty, per_node_beam_size
        self._done = None

    def result(self) -> dict:
        if self._done is not None:
            return self._done
        m, sub = self._m, self._sub

        def extract():
            decoded, logprobs, steps, vis = sub.outs
            dev = self._out_device
            mv = lambda t: t if t is None or t.device == dev else t.to(dev)
            out = {"predictions": mv(decoded), "logprobs": mv(_lp2d(logprobs)),
                   "logits_dict": [] if steps is None else steps, "visual_features": mv(vis)}
            opts = self._opts
            if opts.sampling is not None:
                out["seed"] = opts.sampling[3]
            if opts.prompt is not None:
                out["prompt_lengths"] = mv(opts.prompt.lengths)
            counts = opts.counts
            if counts is not None and vis is not None:       # a ragged batch: packed rows -> the padded pair of the reference
                pv, valid = ragged.unpack_rows(vis, counts, m.cfg.tokens_per_frame)
                out["visual_features"], out["visual_features_valid"] = mv(pv), mv(valid)
            return out

        def rerun():
            if self._opts.counts is not None:                # the packed frames: on the device already, or the callers' host clips again
                fr = sub.frames if sub.parts is None else m._pack_to_device(sub.parts, sub.parts[0].dtype == torch.uint8)
            else:
                fr = m._to_device(sub.rows(0, sub.outs[0].shape[0]))
            sub.outs = m._infer_device(fr, self._opts, sync=True, save_logits=self._save, want_visual=sub.outs[3] is not None, **self._search)
            return extract()

        self._done = self._deliver(extract, self._out_device.type == "cpu", rerun)
        return self._done


class CaptionStream(_WindowStream):
    """Live captioning over a sliding window of frames (GitCaptioner.caption_stream; include/gitcap.h: gitcap_window_*).  Every
    frame is encoded once, when it is pushed; a caption of the last `window` frames re-runs only the decoder's image prefix and the
    token loop.  Captions are bitwise those of greedy_decode (or of infer's device search) on the window's frames.  With a ``gate``
    (gitcap.framegate.FrameGate) only the camera frames it admits are encoded and counted."""

    def __init__(self, model, batch, window, hop, max_len, mode, beam_size, length_penalty, per_node_beam_size, visual_features,
                 gate=None, logprobs=False, num_keep_best=1, repetition_penalty=1.0, sampling=None, prompt=None, constraints=None,
                 carry=False, top_logprobs=0):
        self._beam, self._lp, self._pnb, self._vis = beam_size, length_penalty, per_node_beam_size, visual_features
        # carry: the previous caption (on the device, truncated as it was returned) is the draft of the next window call
        self._carry, self._prev = bool(carry), None
        self._stats = dict(captions=0, draft_tokens=0, accepted=0, tail_steps=0)
        self._sampling = sampling        # (temperature, top_k, top_p, seed | None) of a do_sample stream
        # the stream's prompt (_Prompt | None), constraints (_Constraints | None) and search options: attached again for every caption
        self._attached = (prompt, constraints, None, num_keep_best, repetition_penalty)
        self.last_seed = None            # do_sample: the seed of the caption the last push returned
        self._clear()
        super().__init__(model, WindowSchedule(batch, window, hop), max_len, mode, gate, logprobs, top_logprobs)

    def _reset_lib(self):
        with torch.cuda.device(self._m._dev):
            self._m._call("gitcap_window_reset", self._sched.batch, self._sched.window)

    def _clear(self):
        self._kept = []                  # the last `window` frames per push order, [B, ...] each: what a recovery pushes again
        self._kind = None                # (raw, device) of the frames since the reset
        self._prev = None                # carry: the next caption is a plain call

    def stats(self) -> dict:
        """Since the stream was opened (the student stream's keys): ``captions`` returned, ``draft_tokens`` offered to the verify
        pass (per clip; 0 for a caption decoded by the plain call), ``accepted`` of them (summed over the clips: every clip keeps
        its own), ``tail_steps`` decoded one by one behind a draft, and ``last`` = the same three numbers of the latest caption."""
        return dict(self._stats)

    def _shape(self, frames):
        """[B,H,W,3] uint8 / [B,3,S,S] fp32 (one frame per clip) or [B,n,...] -> (5-D view, raw)."""
        if frames.dim() == 4:
            frames = frames.unsqueeze(1)
        return self._m._check_frames(frames)

    def _push_lib(self, x, raw):
        m = self._m
        fr = m._to_device(x)
        B, n = fr.shape[:2]
        with torch.cuda.device(m._dev):
            if raw:
                m._call("gitcap_window_push_raw", _lib.ptr(fr), B, n, fr.shape[2], fr.shape[3], m._stream())
            else:
                m._call("gitcap_window_push", _lib.ptr(fr), B, n, m._stream())

    def _repush(self):
        """After a failed statistics exchange the library emptied the ring: push the frames it held again (one push)."""
        self._push_lib(torch.stack(self._kept, 1), self._kind[0])

    def _push(self, frames: torch.Tensor, on_cpu: bool):
        """frames: [B,H,W,3] uint8 camera frames or [B,3,S,S] transformed frames, or n of them ([B,n,...]).  -> None, or the caption
        of the window when one is due: greedy ids [B, 1+steps] (truncated as in greedy_decode), or with beam_size the dict infer
        returns.  CPU frames in: the result is on the CPU and vouched for."""
        m = self._m
        x, raw = self._shape(frames)
        B, n = x.shape[:2]
        self._sched.check(B, n)
        kind = (raw, x.device)
        if self._kind is not None and kind != self._kind:
            raise ValueError(f"frames of one window must keep their kind and device ({self._kind} then {kind}); reset() first")
        m._drain()
        failed = False
        try:
            self._push_lib(x, raw)
        except _lib.GitcapExchangeTimeout:
            failed = True
        self._kind = kind
        self._kept = (self._kept + [x[:, i] for i in range(n)])[-self._sched.window:]
        due = self._sched.push(B, n)
        if failed:
            self._repush()
        if not due:
            return None
        try:
            out = self._caption(on_cpu)
            if on_cpu:
                m.poll_errors()
            return out
        except _lib.GitcapExchangeTimeout:        # reported once: the handle has switched to the unfused launches
            self._repush()
            out = self._caption(on_cpu)
            if on_cpu:
                m.poll_errors()
            return out

    def _caption(self, on_cpu):
        m = self._m
        B = self._sched.batch
        vis = tk = None
        if self._vis:
            vis = torch.empty((B, self._sched.window * m.cfg.tokens_per_frame, m.cfg.enc_width), dtype=torch.float32, device=m._dev)
        with torch.cuda.device(m._dev):
            if self._beam is None:
                ids, steps, lp = self._greedy_buffers(B)
                tk = self._topk_buffers(B)
                opts = _CallOptions(m, *self._attached)
                last = dict(draft_tokens=0, accepted=0, tail_steps=0)
                if self._carry and self._prev is not None and self._prev.shape[1] >= 2:
                    last = m._draft_call("gitcap_window_greedy_draft", (), (_lib.ptr(vis),), self._prev, self._max_len, self._mode, ids, steps, lp)
                else:
                    opts.attach(lp, tk)
                    m._call("gitcap_window_greedy", self._max_len, self._mode, _lib.ptr(vis), _lib.ptr(ids), _lib.ptr(steps), m._stream())
            else:
                sampling = m._seeded(self._sampling)
                opts = _CallOptions(m, *self._attached, sampling)
                own, decoded, logprobs = opts.search_outputs(B, self._max_len)
                opts.attach()                    # one-shot: consumed by the search below (a repeated caption attaches again)
                m._call("gitcap_window_beam_search", self._beam, self._max_len, ctypes.c_float(self._lp), self._pnb, _lib.ptr(vis),
                        _lib.ptr(own[0]), _lib.ptr(own[1]), m._stream())
                if sampling is not None:
                    self.last_seed = sampling[3]
        m._last_memory = None
        self._stats["captions"] += 1
        if self._beam is None:
            out = self._finish_greedy(ids, steps, lp, on_cpu, tk)
            if self._carry:
                self._prev = ids[:, :out.shape[1]]
            for k, v in last.items():
                self._stats[k] += v
            self._stats["last"] = last
            return out
        mv = (lambda t: t if t is None else t.cpu()) if on_cpu else (lambda t: t)
        out = {"predictions": mv(decoded), "logprobs": mv(_lp2d(logprobs)), "logits_dict": [], "visual_features": mv(vis)}
        if opts.prompt is not None:
            out["prompt_lengths"] = mv(opts.prompt.lengths)
        return out


def _rebuild(cfg_dict, weights, kwargs):
    return GitCaptioner(GitCapConfig(**cfg_dict), weights, **kwargs)


class GitCaptioner(_NativeModule):
    _PREFIX, _FINALIZE = "gitcap", "gitcap_finalize_weights"

    def __init__(self, cfg: Optional[GitCapConfig] = None, weights: Optional[Mapping[str, np.ndarray]] = None, *,
                 device: str | torch.device = "cuda:0", max_batch: int = 16, max_frames: Optional[int] = None,
                 max_text_len: int = 32, max_beams: int = 1, tokenizer=None, stop: str = "all_sep",
                 weight_dtype: str = "bf16", compute: str = "bf16", fp8_scale: Optional[float] = None, kv_cache: str = "bf16",
                 # constructor kwargs of the reference student (model.py:55-57); only the ids/vocab matter here
                 vocab_length: Optional[int] = None, cls_token_id: Optional[int] = None,
                 sep_token_id: Optional[int] = None, **_ignored_student_kwargs):
        super().__init__()
        cfg = cfg or git_base()
        over = {}
        if vocab_length is not None:
            over["vocab_size"] = int(vocab_length)
        if cls_token_id is not None:
            over["cls_token_id"] = int(cls_token_id)
        if sep_token_id is not None:
            over["sep_token_id"] = int(sep_token_id)
        if over:
            cfg = GitCapConfig(**{**cfg.to_dict(), **over})
        cfg.validate()
        self.cfg = cfg
        self.tokenizer = tokenizer                      # attribute the reference's callers read (inference.py:43)
        self.cls_token_id, self.sep_token_id = cfg.cls_token_id, cfg.sep_token_id
        self.stop = stop
        if weight_dtype not in ("bf16", "fp8_e4m3"):
            raise ValueError("weight_dtype must be 'bf16' or 'fp8_e4m3'")
        self.weight_dtype = weight_dtype
        if compute not in ("bf16", "fp8_ffn"):
            raise ValueError("compute must be 'bf16' or 'fp8_ffn'")
        if compute == "fp8_ffn" and weight_dtype != "fp8_e4m3":
            raise ValueError("compute='fp8_ffn' needs weight_dtype='fp8_e4m3' (the fp8 GEMMs read the e4m3 codes as stored)")
        self.compute = compute
        if fp8_scale is not None and compute != "fp8_ffn":
            raise ValueError("fp8_scale is the activation scale of compute='fp8_ffn'")
        self.fp8_scale = None if fp8_scale is None else float(fp8_scale)
        if kv_cache not in ("bf16", "v_e4m3"):
            raise ValueError("kv_cache must be 'bf16' or 'v_e4m3' (the token loop reads the image prefix's V rows as e4m3 codes)")
        self.kv_cache = kv_cache
        self._kw = dict(max_batch=max_batch, max_frames=max_frames, max_text_len=max_text_len, max_beams=max_beams, stop=stop,
                        weight_dtype=weight_dtype, compute=compute, fp8_scale=fp8_scale, kv_cache=kv_cache)
        self._dev = torch.device(device)
        self._handle = None
        self._weights: Optional[Dict[str, np.ndarray]] = None
        self._last_memory = None
        self._pending, self._pending_key = [], None
        self._inflight = []                             # submissions whose wait has not been enqueued yet (<= 4)
        self._undelivered = set()                       # waited for, but a future has still to hand out (or re-run) its rows
        self._ring = None                               # _StagingRing, made when the first CPU tensor arrives
        self._window_owner = None                       # token of the one live CaptionStream (the handle has one frame window)
        self._pool_owner = None                         # token of the live TeacherStreamPool (state of its own beside the window)
        self.last_accepted: Optional[torch.Tensor] = None   # int32 [B]: draft tokens the last greedy_decode(draft=...) accepted per clip
        self._copy_stream = os.environ.get("GITCAP_COPY_STREAM", "caller")  # "caller" | "own" (A/B switch; see _StagingRing)
        self._lib = _lib.load()                         # raises if libgitcap.so is missing
        self._open()
        if weights is not None:
            self.load_state_dict(weights)

    # ------------------------------------------------------------------ handle management
    def _cconfig(self):
        kw = self._kw
        self.max_batch = int(kw["max_batch"])
        self.max_frames = int(kw["max_frames"] or max(1, self.cfg.num_frames))
        self.max_text_len = int(kw["max_text_len"])
        self.max_beams = int(kw["max_beams"])
        return CGitCapConfig.from_config(self.cfg, self.max_batch, self.max_frames, self.max_text_len, self.max_beams)

    def _configure(self):
        if self.weight_dtype == "fp8_e4m3":     # GEMM weights live in HBM as e4m3 + per-row 2^k scale (half the bytes)
            self._call("gitcap_set_weight_storage", 1)
        if self.compute == "fp8_ffn":           # FC1 / FC2 of the image rows on fp8 MFMA (include/gitcap.h: gitcap_set_compute)
            self._call("gitcap_set_compute", 1)
            if self.fp8_scale is not None:
                self._call("gitcap_set_fp8_scale", ctypes.c_float(self.fp8_scale))
        if self.kv_cache == "v_e4m3":           # image-prefix V as e4m3 codes for the token loop (include/gitcap.h: gitcap_set_kv_cache)
            self._call("gitcap_set_kv_cache", 1)

    def _call(self, name, *args):
        rc = getattr(self._lib, name)(self._handle, *args)
        if rc == _lib.ERR_EXCHANGE:
            # whichever call learns of a failed statistics exchange: every submission whose rows have not been handed out yet
            # (in flight, or already stream-waited by a synchronous call but not delivered) holds undefined ids
            self._poison_inflight()
        self._check(self._handle, rc, name)

    def _staging(self):
        if self._ring is None:
            self._ring = _StagingRing(self._dev, self._lib, own_stream=self._copy_stream == "own")
        return self._ring

    def _submit(self, name, *args, before=None):
        """A gitcap_*_submit call.  If the library reports a failed statistics exchange at this entry (GITCAP_ERR_EXCHANGE, once)
        nothing was submitted: everything already in flight is undefined (marked; each future re-runs its batch when asked) and the
        call is repeated on the handle, which has switched to the unfused launches.  ``before``: a one-shot attachment the call
        consumes (it is made again before the repeat: the refused call consumed the first)."""
        try:
            if before is not None:
                before()
            self._call(name, *args)
        except _lib.GitcapExchangeTimeout:
            self._poison_inflight()
            if before is not None:
                before()
            self._call(name, *args)

    def poll_errors(self):
        """Raises GitcapExchangeTimeout if a fused GEMM + LayerNorm launch gave up waiting since the last check
        (gitcap_poll_errors, include/gitcap.h).  Meaningful after the stream that produced a result was synchronised."""
        self._call("gitcap_poll_errors")

    def _vouched(self, produce):
        """Run `produce()` (which must end in a host synchronisation, e.g. a copy to the CPU) and vouch for its result:
        if the exchange flag was raised meanwhile -- at entry, for earlier work, or by this very call -- the library has
        switched to the unfused launches and the call is repeated once on those."""
        try:
            out = produce()
            self.poll_errors()
            return out
        except _lib.GitcapExchangeTimeout:
            self._poison_inflight()          # their ids are undefined: each future re-runs its batch when asked for its result
            out = produce()
            self.poll_errors()
            return out

    # ------------------------------------------------------------------ submissions in flight
    def _wait_submission(self, sub):
        """Make the current stream wait for a submission (once).  Its frames/ids/steps buffers are owned by the
        model-side table until then: dropping a future early cannot hand them back to the allocator while the
        library's streams still read frames / write ids."""
        if not sub.waited and not sub.poisoned:
            try:
                with torch.cuda.device(self._dev):
                    self._call("gitcap_greedy_wait", sub.ticket, self._stream())
                    sub.done_ev = torch.cuda.Event()
                    sub.done_ev.record(torch.cuda.current_stream(self._dev))
                sub.waited = True
            except _lib.GitcapExchangeTimeout:   # raised now, or this ticket was in flight when it was raised: everything
                self._poison_inflight()          # submitted so far is undefined (the C ABI marks the same tickets)
                sub.poisoned = True
        if sub in self._inflight:
            self._inflight.remove(sub)
            if sub.users > 0:                    # until every future has delivered, a failure reported later still marks it
                sub.owner = self
                self._undelivered.add(sub)

    def _poison_inflight(self):
        for sub in self._inflight:
            sub.poisoned = True
        for sub in self._undelivered:            # stream-waited (e.g. by a synchronous call's _drain) but not handed out yet
            sub.poisoned = True

    def _drain(self):
        """Before a synchronous call: submit what is still waiting to coalesce and order the current stream behind
        every submission in flight (the C ABI orders the device work as well; this releases the buffers)."""
        if self._pending:
            self._flush_pending()
        for sub in list(self._inflight):
            self._wait_submission(sub)

    # ------------------------------------------------------------------ nn.Module surface
    def to(self, *args, **kwargs):
        self._window_owner = None                       # a CaptionStream does not follow the model
        self._pool_owner = None                         # nor does a TeacherStreamPool
        return super().to(*args, **kwargs)

    def cuda(self, device=None):
        return self.to(torch.device("cuda", device if device is not None else torch.cuda.current_device()))

    def load_state_dict(self, state_dict, strict: bool = True):
        """Accepts canonical names (gitcap/weights.py), a transformers GitForCausalLM state dict or the
        MS GenerativeImage2Text checkpoint layout the reference loads (model.py:736-738)."""
        keys = state_dict.keys()
        if "enc.patch_w" in keys:
            w = {k: self._as_f32(v) for k, v in state_dict.items()}
            W.check_shapes(self.cfg, w)
        elif any(k.startswith("git.") for k in keys):
            w = W.from_hf_state_dict(self.cfg, state_dict)
        elif any(k.startswith("image_encoder.") for k in keys):
            w = W.from_ms_state_dict(self.cfg, state_dict)
        else:
            raise KeyError("unrecognised checkpoint layout (expected canonical, HF-GIT or MS-GIT keys)")
        if self.weight_dtype == "fp8_e4m3":      # BASELINE configs[4]: fp8 (e4m3) weight values, per-row 2^k scale
            w = W.quantize_weights_fp8(w)
        self._upload(w)
        self._weights = w
        return self

    def _upload(self, w: Mapping[str, np.ndarray]):
        self._pool_owner = None                         # the pool's rows came from the old encoder weights
        self._load_tensors((name, w[name]) for name in W.canonical_shapes(self.cfg))

    def __reduce__(self):
        kw = dict(self._kw)
        kw["device"] = str(self._dev)
        return _rebuild, (self.cfg.to_dict(), self._weights, kw)

    # ------------------------------------------------------------------ helpers
    def _check_frames(self, x: torch.Tensor):
        """Shape checks only (nothing is moved): -> (5-D view, raw) with raw = uint8 BGR camera frames [B,F,H,W,3] (OpenCV layout,
        real_time_inference.py:39; [F,H,W,3] = one clip) as opposed to transformed frames [B,F,3,S,S] ([B,3,S,S] = one frame each)."""
        raw = x.dtype == torch.uint8
        if raw:
            if x.dim() == 4:
                x = x.unsqueeze(0)
            if x.dim() != 5 or x.shape[-1] != 3:
                raise ValueError(f"expected uint8 frames [B,F,H,W,3], got {tuple(x.shape)}")
            if min(x.shape[2], x.shape[3]) < 1:
                raise ValueError("empty frames")
        else:
            if x.dim() == 4:                                  # [B,3,H,W] single image -> one frame
                x = x.unsqueeze(1)
            if x.dim() != 5 or x.shape[2] != 3 or x.shape[3] != self.cfg.image_size or x.shape[4] != self.cfg.image_size:
                raise ValueError(f"expected frames [B,F,3,{self.cfg.image_size},{self.cfg.image_size}], got {tuple(x.shape)}")
        if x.shape[0] == 0:
            raise ValueError("empty batch")
        if x.shape[1] > self.max_frames:
            raise ValueError(f"{x.shape[1]} frames per clip > max_frames={self.max_frames}")
        return x, raw

    def _to_device(self, x: torch.Tensor) -> torch.Tensor:
        """Checked frames -> contiguous, 16-byte aligned device tensor (fp32 NCHW or uint8 HWC) for a SYNCHRONOUS call.  A CPU
        tensor (real_time_inference.py:57) goes through the pinned staging entry of the synchronous calls on the current stream
        (a pageable x.to(device) is a blocking, runtime-staged copy)."""
        dtype = torch.uint8 if x.dtype == torch.uint8 else torch.float32
        if x.device.type == "cpu":
            with torch.cuda.device(self._dev):
                dv, _, _ = self._staging().stage(self, [x], dtype, stream=torch.cuda.current_stream(self._dev))
            return dv
        x = x.to(device=self._dev, dtype=dtype).contiguous()
        if x.data_ptr() % 16:
            x = x.clone()
        return x

    def _frames(self, x: torch.Tensor) -> torch.Tensor:
        x, raw = self._check_frames(x)
        if raw:
            raise ValueError("this call takes transformed fp32 frames [B,F,3,S,S], not uint8 camera frames")
        return self._to_device(x)

    def _raw_frames(self, x: torch.Tensor) -> torch.Tensor:
        """uint8 BGR camera frames [B,F,H,W,3] (OpenCV layout, real_time_inference.py:39) or [F,H,W,3] for one clip."""
        x, raw = self._check_frames(x)
        if not raw:
            raise ValueError(f"expected uint8 frames [B,F,H,W,3], got {x.dtype}")
        return self._to_device(x)

    def _constraints(self, no_repeat_ngram_size, min_length, suppress_tokens, max_len, need=1):
        """The constraint arguments of the decoding calls -> _Constraints or None (the defaults: nothing is attached).  ValueError
        for what the library would refuse (include/gitcap.h: gitcap_attach_constraints), before anything is launched."""
        from .search import check_constraints
        n, m, sup = check_constraints(no_repeat_ngram_size, min_length, suppress_tokens)
        if not (n or m or sup):
            return None
        if len(sup) + max_len + need > self.cfg.vocab_size:
            raise ValueError(f"{len(sup)} suppressed ids over {max_len} steps could ban every column of a row (vocab_size {self.cfg.vocab_size})")
        return _Constraints(self, n, m, sup)

    def _ids(self, y: torch.Tensor) -> torch.Tensor:
        return y.to(device=self._dev, dtype=torch.int64).contiguous()

    # ------------------------------------------------------------------ ragged batches (frame_counts=; gitcap/ragged.py)
    def _frame_limit(self) -> int:
        nf = self.cfg.num_frames
        return min(self.max_frames, nf) if nf > 0 else self.max_frames

    def _ragged_input(self, src, frame_counts):
        """``src`` + ``frame_counts`` of a decoding call -> (dense tensor [B, F, ...], None) when every clip has the same number
        of frames (the existing path: nothing is attached) or (None, (clips, counts, raw)) for a ragged batch."""
        parts, counts, raw = ragged.clips(src, frame_counts, self.cfg.image_size, self._frame_limit())
        if ragged.is_dense(counts):
            return ragged.dense(parts), None
        return None, (parts, counts, raw)

    def _pack_to_device(self, parts, raw) -> torch.Tensor:
        """The clips of a ragged (chunk of a) batch -> packed device frames [sum(counts), ...] for a SYNCHRONOUS call: one
        packing copy, for host clips into the pinned staging entry of the synchronous calls (as _to_device)."""
        dtype = torch.uint8 if raw else torch.float32
        if parts[0].device.type == "cpu":
            with torch.cuda.device(self._dev):
                dv, _, _ = self._staging().stage(self, list(parts), dtype, stream=torch.cuda.current_stream(self._dev))
            return dv
        x = ragged.pack(parts).to(device=self._dev, dtype=dtype).contiguous()
        if x.data_ptr() % 16:
            x = x.clone()
        return x

    def _attach_counts(self, counts):
        """The one-shot attachment the NEXT call with an image pass consumes (gitcap_attach_frame_counts; the counts are copied)."""
        self._call("gitcap_attach_frame_counts", (ctypes.c_int32 * len(counts))(*counts), len(counts))

    def _encode_ragged(self, parts, counts, raw) -> torch.Tensor:
        """The image pass of one ragged batch of at most max_batch clips -> the packed fp32 visual rows [sum(counts) * N, Dv];
        leaves the decoder's image K/V (and the slot's row tables) in the handle."""
        if len(counts) > self.max_batch:
            raise ValueError(f"batch {len(counts)} > max_batch={self.max_batch}")
        fr = self._pack_to_device(parts, raw)
        vis = torch.empty((fr.shape[0] * self.cfg.tokens_per_frame, self.cfg.enc_width), dtype=torch.float32, device=self._dev)
        with torch.cuda.device(self._dev):
            self._attach_counts(counts)
            if raw:
                self._call("gitcap_encode_raw", _lib.ptr(fr), len(counts), max(counts), fr.shape[1], fr.shape[2], _lib.ptr(vis), self._stream())
            else:
                self._call("gitcap_encode", _lib.ptr(fr), len(counts), max(counts), _lib.ptr(vis), self._stream())
        self._last_memory = None
        return vis

    # ------------------------------------------------------------------ reference API
    @torch.no_grad()
    def forward_image_enc(self, x: torch.Tensor, frame_counts=None):
        """-> ([], memory) with memory = visual features [B, F*N, Dv] (ln_post + temporal embedding,
        frames concatenated along tokens, model.py:378-382).  Also leaves the decoder's image K/V
        in the handle.
        frame_counts (or ``x`` as a list of B clips [F_b, ...]): clips that differ in length -> (visual [B, Fmax*N, Dv], zero
        beyond a clip's rows, valid bool [B, Fmax*N]): the reference's visual_features / visual_features_valid pair
        (model.py:426, :443).  The handle then holds the batch packed; score / forward_decoder-style calls follow it."""
        self._drain()
        if frame_counts is not None or not isinstance(x, torch.Tensor):
            x, rg = self._ragged_input(x, frame_counts)
            if rg is not None:
                parts, counts, raw = rg
                return ragged.unpack_rows(self._encode_ragged(parts, counts, raw), counts, self.cfg.tokens_per_frame)
            vis = self.forward_image_enc(x)[1]
            return vis, torch.ones(vis.shape[:2], dtype=torch.bool, device=vis.device)
        raw = x.dtype == torch.uint8
        fr = self._raw_frames(x) if raw else self._frames(x)
        B, F = fr.shape[:2]
        if B > self.max_batch:
            raise ValueError(f"batch {B} > max_batch={self.max_batch} (use greedy_decode for automatic chunking)")
        vis = torch.empty((B, F * self.cfg.tokens_per_frame, self.cfg.enc_width), dtype=torch.float32, device=self._dev)
        with torch.cuda.device(self._dev):
            if raw:
                self._call("gitcap_encode_raw", _lib.ptr(fr), B, F, fr.shape[2], fr.shape[3], _lib.ptr(vis), self._stream())
            else:
                self._call("gitcap_encode", _lib.ptr(fr), B, F, _lib.ptr(vis), self._stream())
        self._remember_memory(vis)
        return [], vis

    def _remember_memory(self, t: torch.Tensor):
        # identity (a weak reference that dies with the tensor) + version: a recycled address cannot alias it
        self._last_memory = (weakref.ref(t), t._version)

    def _is_last_memory(self, t: torch.Tensor) -> bool:
        lm = self._last_memory
        return lm is not None and lm[0]() is t and lm[1] == t._version

    @torch.no_grad()
    def forward_decoder(self, y: torch.Tensor, memory: torch.Tensor) -> torch.Tensor:
        """Teacher-forced logits [B,T,V] for token prefixes y [B,T] given `memory` from
        forward_image_enc (block mask: text->image full, text->text causal)."""
        self._drain()
        ids = self._ids(y)
        B, T = ids.shape
        with torch.cuda.device(self._dev):
            if not self._is_last_memory(memory):
                mem = memory.to(device=self._dev, dtype=torch.float32).contiguous()
                self._call("gitcap_set_visual", _lib.ptr(mem), mem.shape[0], mem.shape[1], self._stream())
                self._remember_memory(memory)
            logits = torch.empty((B, T, self.cfg.vocab_size), dtype=torch.float32, device=self._dev)
            self._call("gitcap_text_forward", _lib.ptr(ids), T, B, 1, 0, T, _lib.ptr(logits), 1, None, 0, self._stream())
        return logits

    @torch.no_grad()
    def score(self, x: torch.Tensor, y: torch.Tensor, *, lengths: Optional[torch.Tensor] = None, until_sep: bool = True,
              ignore_id: Optional[int] = None, return_top1: bool = False, frame_counts=None, top_k: int = 0) -> dict:
        """Log-probabilities of GIVEN captions, teacher-forced in one pass without a logits tensor (include/gitcap.h:
        gitcap_score).  ``x``: frames [B,F,3,S,S] or ``memory`` from forward_image_enc (treated as forward_decoder treats it);
        ``y``: CLS-first ids [B, T] or [B, n, T] -- n candidates per clip, run as n rows that share the clip's image K/V.
        A position is ignored (log-probability 0, not counted) when its target is outside the vocabulary, equals ``ignore_id``,
        or lies behind the row's length: through its first SEP (``until_sep``) and / or the caller's ``lengths`` ([B] or [B, n],
        valid tokens, CLS included).  -> dict: ``token_logprobs`` fp32 [B, (n,) T-1] (column j belongs to y[..., j + 1]),
        ``sum`` fp32 and ``count`` int32 [B, (n)]; with ``return_top1`` also ``top1_ids`` / ``top1_logprobs`` [B, (n,) T-1], the
        model's own arg-max at each position.  More clips than max_batch go through in chunks.  On ``x``'s device.
        frame_counts (or ``x`` as a list of clips; as in greedy_decode): frames of clips that differ in length; every clip's values
        are bit for bit those of the clip scored alone.
        top_k=k (1..32): also ``topk_ids`` int64 / ``topk_logprobs`` fp32 [B, (n,) T-1, k], the model's k best tokens at every
        position (ignored ones included) ranked by (logit descending, id ascending): rank 0 is top1_ids / top1_logprobs bit for
        bit, and the values are those of greedy_decode(top_logprobs=k) for the same prefix (gitcap_attach_top_logprobs)."""
        from . import scoring
        top_k = scoring.check_top_k(top_k)
        self._drain()
        ids, had_n = scoring.candidates(y, self._dev)
        B, n, T = ids.shape
        rg = None
        if frame_counts is not None or not isinstance(x, torch.Tensor):
            x, rg = self._ragged_input(x, frame_counts)
        if (x.shape[0] if rg is None else len(rg[1])) != B:
            raise ValueError("x and y disagree on the number of clips")
        if T > self.max_text_len:
            raise ValueError(f"T={T} > max_text_len={self.max_text_len} the handle was created for")
        Bc = min(B, self.max_batch)
        if Bc * n > self.max_batch * self.max_beams:
            raise ValueError(f"{Bc} clips x {n} candidates = {Bc * n} rows > max_batch * max_beams = {self.max_batch * self.max_beams} "
                             "the handle was created for")
        ln = scoring.row_lengths(ids, self.sep_token_id, until_sep, lengths)
        frames = rg is None and x.dim() == 5
        out_dev = x.device if rg is None else rg[0][0].device
        chunks = []
        with torch.cuda.device(self._dev):
            for b0 in range(0, B, Bc):
                b1 = min(B, b0 + Bc)
                if rg is not None:
                    self._encode_ragged(rg[0][b0:b1], rg[1][b0:b1], rg[2])
                elif frames:
                    self.forward_image_enc(x[b0:b1])
                elif not (b0 == 0 and b1 == B and self._is_last_memory(x)):
                    mem = x[b0:b1].to(device=self._dev, dtype=torch.float32).contiguous()
                    self._call("gitcap_set_visual", _lib.ptr(mem), mem.shape[0], mem.shape[1], self._stream())
                    self._last_memory = None
                    if b0 == 0 and b1 == B:
                        self._remember_memory(x)
                rows = (b1 - b0) * n
                buf = scoring.ScoreBuffers(rows, T, self._dev, return_top1, top_k)
                cid = ids[b0:b1].reshape(rows, T)
                cl = None if ln is None else ln[b0:b1].reshape(rows).contiguous()
                buf.attach_topk(self._call, "gitcap_attach_top_logprobs")
                self._call("gitcap_score", _lib.ptr(cid), T, rows, n, T, _lib.ptr(cl), -1 if ignore_id is None else int(ignore_id),
                           *buf.args(T), self._stream())
                chunks.append(buf)
        if B > Bc:
            self._last_memory = None
        return scoring.result(chunks, B, n, had_n, return_top1, out_dev)

    @torch.no_grad()
    def attention(self, x: torch.Tensor, y: torch.Tensor, *, layer: Optional[int] = None, patches: bool = False,
                  lengths: Optional[torch.Tensor] = None, until_sep: bool = True, frame_counts=None) -> dict:
        """Which frames and patches every token of GIVEN captions comes from: the decoder's attention probabilities, averaged over
        the heads and over all layers (``layer=None``) or one (``layer=l``), read back from the K/V cache of score's pass
        (include/gitcap.h: gitcap_attention_map).  ``x``, ``y``, ``lengths``, ``until_sep``, ``frame_counts`` as in score.
        -> dict: ``frame_attention`` fp32 [B, (n,) T-1, Fmax], the probability mass on each frame's image tokens (0 for frames a
        clip of a ragged batch does not have); ``text_attention`` fp32 [B, (n,) T-1], the mass on the caption's own tokens (the
        two sum to 1); with ``patches`` also ``patch_attention`` fp32 [B, (n,) T-1, Fmax, N], the mean probability of every image
        token (N per frame, the class token first).  Index j is the position that predicts y[..., j + 1], as in score; positions
        behind a row's length hold zeros.  Every clip's values are bit for bit those of the clip alone, and those of
        greedy_decode(return_attention=True) for the same tokens."""
        from . import scoring
        ids, had_n = scoring.candidates(y, self._dev)
        B, n, T = ids.shape
        if T < 2:
            raise ValueError("attention needs CLS and at least one token")
        lay = -1 if layer is None else int(layer)
        if not -1 <= lay < self.cfg.dec_layers:
            raise ValueError(f"layer={layer} outside 0..{self.cfg.dec_layers - 1}")
        ln = scoring.row_lengths(ids, self.sep_token_id, until_sep, lengths)
        Bc = min(B, self.max_batch)
        N = (self.cfg.image_size // self.cfg.patch_size) ** 2 + 1
        fms, tms, pms = [], [], []
        # score's pass chunk by chunk (its outputs are not kept), the maps behind each chunk from the cache it filled
        for b0 in range(0, B, Bc):
            b1 = min(B, b0 + Bc)
            xs = x[b0:b1] if isinstance(x, torch.Tensor) else x[b0:b1]
            fc = None if frame_counts is None else frame_counts[b0:b1]
            self.score(xs, ids[b0:b1] if had_n else ids[b0:b1, 0], lengths=None if ln is None else (ln[b0:b1] if had_n else ln[b0:b1, 0]),
                       until_sep=False, frame_counts=fc)
            rows = (b1 - b0) * n
            with torch.cuda.device(self._dev):
                if fc is not None:
                    F = int(max(int(c) for c in fc))
                elif not isinstance(x, torch.Tensor):
                    F = max(int(c.shape[0]) for c in xs)
                else:
                    F = int(x.shape[1]) if x.dim() == 5 else int(x.shape[1]) // N
                fm = torch.empty((rows, T - 1, F), dtype=torch.float32, device=self._dev)
                tm = torch.empty((rows, T - 1), dtype=torch.float32, device=self._dev)
                pm = torch.empty((rows, T - 1, F * N), dtype=torch.float32, device=self._dev) if patches else None
                cl = None if ln is None else (ln[b0:b1].reshape(rows) - 1).clamp_(min=0).to(torch.int32).contiguous()
                self._call("gitcap_attention_map", rows, T - 1, lay, _lib.ptr(cl), _lib.ptr(fm), F, _lib.ptr(tm), _lib.ptr(pm), F * N,
                           self._stream())
            fms.append(fm)
            tms.append(tm)
            pms.append(pm)
        out_dev = x.device if isinstance(x, torch.Tensor) else x[0].device
        Fmax = max(f.shape[2] for f in fms)
        pad = lambda t, w: t if t.shape[2] == w else torch.nn.functional.pad(t, (0, w - t.shape[2]))
        shape = (B, n) if had_n else (B,)
        out = dict(frame_attention=torch.cat([pad(f, Fmax) for f in fms], 0).reshape(*shape, T - 1, Fmax).to(out_dev),
                   text_attention=torch.cat(tms, 0).reshape(*shape, T - 1).to(out_dev))
        if patches:
            out["patch_attention"] = torch.cat([pad(p, Fmax * N) for p in pms], 0).reshape(*shape, T - 1, Fmax, N).to(out_dev)
        return out

    @torch.no_grad()
    def rerank(self, x: torch.Tensor, candidates: torch.Tensor, length_penalty: float = 0.6, frame_counts=None) -> dict:
        """Order n candidate captions per clip ([B, n, T], e.g. infer(num_keep_best=n), sampled captions, the student's beams)
        by this model's sum / count ** length_penalty, the BeamHypotheses score of the reference's search.  -> score()'s dict
        plus ``scores`` fp32 [B, n] and ``order`` int64 [B, n], best first."""
        from . import scoring
        if candidates.dim() != 3:
            raise ValueError(f"expected candidates [B, n, T], got {tuple(candidates.shape)}")
        return scoring.rerank_scores(self.score(x, candidates, frame_counts=frame_counts), length_penalty)

    def forward(self, x: torch.Tensor, y: Optional[torch.Tensor] = None, frame_counts=None):
        """``forward(x, y)``: teacher-forced logits [B,T,V] (student signature, model.py:99-106).
        ``forward(x)``: the teacher's form (``GenerativeImageTextTeacher.forward``, model.py:762-793).
        frame_counts (or ``x`` as a list of clips): clips that differ in length, as in greedy_decode."""
        if y is None:
            return self.teacher_forward(x, frame_counts=frame_counts)
        if frame_counts is not None or not isinstance(x, torch.Tensor):
            self._drain()
            x, rg = self._ragged_input(x, frame_counts)
            if rg is not None:                   # the handle holds the packed batch: the text rows follow its tables
                self._encode_ragged(*rg)
                ids = self._ids(y)
                B, T = ids.shape
                if B != len(rg[1]):
                    raise ValueError("x and y disagree on the number of clips")
                logits = torch.empty((B, T, self.cfg.vocab_size), dtype=torch.float32, device=self._dev)
                with torch.cuda.device(self._dev):
                    self._call("gitcap_text_forward", _lib.ptr(ids), T, B, 1, 0, T, _lib.ptr(logits), 1, None, 0, self._stream())
                return logits
        _, memory = self.forward_image_enc(x)
        return self.forward_decoder(y, memory)

    @torch.no_grad()
    def teacher_forward(self, x: torch.Tensor, beam_size: int = 4, max_steps: int = 15, on_device: Optional[bool] = None,
                        frame_counts=None) -> list:
        """``GenerativeImageTextTeacher.forward`` (model.py:762-793): one dict per clip with the keys of
        ``infer`` (model.py:456-461) plus ``cap`` (decoded caption, :770) and ``output`` [1, n, V] = for each of
        the first n predicted words the logits of the beam that scores that word highest (:771-788).
        The reference runs one clip at a time (:765); here the clips go through batched searches (chunks of max_batch, pipelined:
        the image pass of one chunk overlaps the search of the one before) and only the per-clip bookkeeping is a loop.  Default:
        the device-resident search with its per-step logits kept on the device (``infer_async``); on_device=False: the host-side
        operator (one host sync per step).  ``logits_dict`` holds every step's [beams, V] logits; the device search runs all
        max_steps - 1 steps where the reference stops once the clip is done (:640) -- ``output`` only reads the first n.
        Without a tokenizer ``cap`` is None and n counts the tokens before SEP."""
        if on_device is None:
            on_device = beam_size * 2 <= 16
        rg = None
        if frame_counts is not None or not isinstance(x, torch.Tensor):
            x, rg = self._ragged_input(x, frame_counts)
        if rg is not None:                        # clips that differ in length: fr = the list of clips, a chunk = a ragged batch
            fr, nclips, rkw = rg[0], len(rg[1]), {"frame_counts": None}
        else:
            fr, _ = self._check_frames(x)         # a CPU tensor stays where it is: every chunk is staged as it is submitted
            nclips, rkw = fr.shape[0], {}
        out = []

        def finish(pred, pred_h, logprobs, steps, vis):       # per-clip bookkeeping of one chunk; steps: [S, Bc * beams, V] on the device
            for b in range(pred.shape[0]):
                dist_all = steps[:, b * beam_size:(b + 1) * beam_size]              # [S, beams, V]
                ids = pred_h[b].tolist()
                if self.tokenizer is not None:
                    cap = self.tokenizer.decode(ids, skip_special_tokens=True)
                    n = min(len(cap.split(" ")), dist_all.shape[0])                 # model.py:771
                else:
                    cap = None
                    body = ids[1:]
                    n = min(body.index(self.sep_token_id) if self.sep_token_id in body else len(body), dist_all.shape[0])
                n = max(n, 1)
                dist = dist_all[:n]                                                 # [n, beams, V]
                words = pred[b, 1:n + 1].to(self._dev)
                at_word = torch.gather(dist, 2, words[:, None, None].expand(-1, beam_size, -1)).squeeze(-1)   # [n, beams]
                best = at_word.argmax(dim=1)                                        # model.py:785
                output = torch.gather(dist, 1, best[:, None, None].expand(-1, -1, dist.shape[-1])).squeeze(1)[None]
                out.append({"predictions": pred[b:b + 1], "logprobs": logprobs[b:b + 1],
                            "logits_dict": [a for a in dist_all.cpu().numpy()],
                            "visual_features": vis[b:b + 1], "output": output, "cap": cap})

        if on_device:
            # a sliding window of submissions, each consumed (and its [max_steps - 1, B * beams, V] logits tensor dropped) before
            # the next is made: device memory is bounded by the window, not by the number of chunks
            kw = dict(beam_size=beam_size, max_steps=max_steps, save_logits=True, visual_features=True, **rkw)
            futs = []

            def take(f, b0):
                r = f.result()
                pred_h = r["predictions"].cpu()           # a host synchronisation: the result can be vouched for now
                try:
                    self.poll_errors()
                except _lib.GitcapExchangeTimeout:        # (the failure poisoned what is in flight; this chunk is re-run here)
                    r = self.infer_async(fr[b0:b0 + self.max_batch], **kw).result()
                    pred_h = r["predictions"].cpu()
                    self.poll_errors()
                finish(r["predictions"], pred_h, r["logprobs"], r["logits_dict"], r["visual_features"])

            for b0 in range(0, nclips, self.max_batch):
                if len(futs) >= 3:
                    take(*futs.pop(0))
                futs.append((self.infer_async(fr[b0:b0 + self.max_batch], **kw), b0))
            while futs:
                take(*futs.pop(0))
        else:
            for b0 in range(0, nclips, 1 if rg is not None else self.max_batch):      # (ragged: clip by clip, as the reference, model.py:765)
                xb = fr[b0][None] if rg is not None else fr[b0:b0 + self.max_batch]
                r = self.infer(xb, beam_size=beam_size, max_steps=max_steps, save_logits=True, on_device=False)
                steps = torch.from_numpy(np.stack([np.asarray(st) for st in r["logits_dict"]])).to(self._dev)
                finish(r["predictions"], r["predictions"].cpu(), r["logprobs"], steps, r["visual_features"])
        return out

    @torch.no_grad()
    def forward_output_logits(self, x: torch.Tensor, y: torch.Tensor, output_hidden_states: bool = False):
        """Teacher API (model.py:747-760): per clip lists of logits [1,T,V], visual features [1,F*N,Dv] and hidden
        states; computed as ONE batch instead of the reference's clip-by-clip loop (:752-759).
        The third list (model.py:419-424: the decoder stack's per-layer hidden states over [image ; text], stacked
        to [dec_layers + 1, F*N + T, D] per clip) is opt-in: the reference's only caller discards it (:896) and it costs
        a copy of every row after every layer plus the image rows of the last layer.  Empty unless requested."""
        if not output_hidden_states:
            _, vis = self.forward_image_enc(x)
            logits = self.forward_decoder(y, vis)
            return [l[None] for l in logits], [v[None] for v in vis], []
        self._drain()
        self._call("gitcap_hidden_states_enable", 1)
        try:
            _, vis = self.forward_image_enc(x)
            logits = self.forward_decoder(y, vis)
            B, S_img, T = vis.shape[0], vis.shape[1], logits.shape[1]
            hid = torch.empty((B, self.cfg.dec_layers + 1, S_img + T, self.cfg.dec_width), dtype=torch.float32, device=self._dev)
            with torch.cuda.device(self._dev):
                self._call("gitcap_hidden_states_read", B, S_img, T, _lib.ptr(hid), self._stream())
        finally:
            self._call("gitcap_hidden_states_enable", 0)
            self._last_memory = None
        return [l[None] for l in logits], [v[None] for v in vis], [h for h in hid]

    @torch.no_grad()
    def greedy_decode(self, src: torch.Tensor, max_len: int = 10, stop: Optional[str] = None, return_logprobs: bool = False,
                      prompt=None, prompt_lengths=None, no_repeat_ngram_size: int = 0, min_length: int = 0, suppress_tokens=None,
                      frame_counts=None, draft: Optional[torch.Tensor] = None, top_logprobs: int = 0, return_attention: bool = False):
        """CLS-prefixed greedy ids [B, 1+steps] (model.py:156-187).  stop='all_sep' is the
        reference rule (break when every row emits SEP in the same step, :184); 'never' always
        runs max_len steps.  The loop runs on the device without per-step host syncs; the
        truncation the reference's `break` implies is applied afterwards.  return_logprobs=True: (ids, logprobs), logprobs fp32
        [B, steps] on src's device, column t = log_softmax(step t's logits)[ids[:, t + 1]] (include/gitcap.h:
        gitcap_attach_token_logprobs; the ids are the same either way).
        prompt: per-clip text prefixes the captions start from (the `prefix` branch of model.py:432-437; include/gitcap.h:
        gitcap_attach_prompt): int64 [B, P], optionally with prompt_lengths [B], or a list of B 1-D tensors of different lengths;
        CLS is prepended where a row does not start with it.  The ids returned INCLUDE each row's prompt (columns
        0 .. its length - 1; the reference strips its single prefix, :455, which a ragged batch cannot do); prompt tokens do not
        count for stop='all_sep', and their logprobs columns are 0.
        no_repeat_ngram_size / min_length / suppress_tokens: hard constraints on what a step may emit (include/gitcap.h:
        gitcap_attach_constraints; HF's NoRepeatNGram / MinLength / SuppressTokens processors): no n-gram of the row so far (CLS
        and prompt included) may recur, SEP is banned while the row holds fewer than min_length tokens, the listed ids (a sequence
        or an int tensor, at most 256) are never emitted.  A banned column is -inf inside the vocabulary head, so the logprobs
        are those of the row renormalised over the allowed columns; a token a prompt forces is emitted even when banned.  With
        the defaults nothing is attached.
        frame_counts: clips that differ in length -- ``src`` padded [B, Fmax, ...] with frame_counts [B] (frames beyond a clip's
        count are ignored) or a list of B clips [F_b, ...] (counts inferred); fp32 or uint8 camera frames, host or device.  The
        batch runs packed, without padding or masking (include/gitcap.h: gitcap_attach_frame_counts): every clip's ids and
        logprobs are bit for bit those of the clip decoded alone.  Equal counts take the dense path.
        draft: int64 [B, 1+n], a guess at the result (the previous caption of a live stream, the student's caption of the same
        frames; column 0 is taken as CLS, any ids are allowed).  The result is the one without it, bit for bit: the draft is
        verified in one pass, every clip keeps the leading tokens the loop would have produced anyway (``last_accepted`` [B] =
        their numbers) and only the steps some clip still lacks are decoded one by one (include/gitcap.h: gitcap_greedy_draft).
        The call waits on the host for the verify pass.  Not with prompt or the constraint arguments.
        top_logprobs=k (1..32): the result gains ``top_ids`` int64 and ``top_logprobs`` fp32 [B, steps, k] behind ids (and behind
        logprobs with return_logprobs): the k best tokens of the distribution each step chose from and their log-probabilities,
        ranked by (logit descending, id ascending); rank 0 is the emitted token (its value == the logprobs column) except at a
        position a prompt forces, which reports the model's own ranks.  Ranks a row cannot fill (bans) hold -1 / -inf.  No
        logits tensor is written (include/gitcap.h: gitcap_attach_top_logprobs).  A ``draft`` call refuses it.
        return_attention=True: the result gains, last, ``frame_attention`` fp32 [B, steps, Fmax] and ``text_attention`` fp32
        [B, steps]: per emitted token the attention mass on each frame and on the caption so far, averaged over heads and
        layers (see attention()), read from the K/V cache the loop just filled -- no extra pass; bit for bit attention(x, ids).
        Not with ``draft``."""
        if not 0 <= int(top_logprobs) <= 32:
            raise ValueError(f"top_logprobs={top_logprobs} outside 0..32")
        if return_attention and draft is not None:
            raise ValueError("return_attention= is not combined with draft= (use attention(x, ids) on the result)")
        if draft is not None and (prompt is not None or no_repeat_ngram_size or min_length or suppress_tokens is not None):
            raise ValueError("draft= is not combined with prompt= or the constraint arguments")
        stop = stop or self.stop
        mode = {"all_sep": STOP_ALL_SEP, "never": STOP_NEVER}[stop]
        if max_len > self.max_text_len:
            raise ValueError(f"max_len {max_len} > max_text_len={self.max_text_len} the handle was created for")
        rg = None
        if frame_counts is not None or not isinstance(src, torch.Tensor):
            src, rg = self._ragged_input(src, frame_counts)
        B, in_dev = (src.shape[0], src.device) if rg is None else (len(rg[1]), rg[0][0].device)
        opts = self._greedy_options(B, max_len, prompt, prompt_lengths, no_repeat_ngram_size, min_length, suppress_tokens, rg)
        opts.top_k = int(top_logprobs)
        if draft is not None and (draft.dim() != 2 or draft.shape[0] != B or draft.shape[1] < 2 or draft.dtype != torch.int64):
            raise ValueError(f"draft must be int64 [{B}, 1+n] with n >= 1, got {draft.dtype} {tuple(draft.shape)}")
        if in_dev.type == "cpu":                  # CPU tensor in -> CPU ids out (real_time_inference.py:57): the copy back is a
            return self._vouched(lambda: self._greedy_decode(src, max_len, mode, return_logprobs, opts, rg, draft, return_attention))    # synchronisation, so the result is vouched for
        return self._greedy_decode(src, max_len, mode, return_logprobs, opts, rg, draft, return_attention)

    def _greedy_options(self, B, max_len, prompt, prompt_lengths, no_repeat_ngram_size, min_length, suppress_tokens, rg=None):
        """The option arguments of the greedy calls (rg: the ragged batch, or None) -> _CallOptions"""
        return _CallOptions(self, self._prompt(prompt, prompt_lengths, B, max_len, "max_len"),
                            self._constraints(no_repeat_ngram_size, min_length, suppress_tokens, max_len), None if rg is None else rg[1])

    def _chunks(self, fr, rg):
        """A synchronous call's input in chunks of at most max_batch clips -> (first clip, nb, F, fh, fw, device frames) each: fr the
        checked dense frames [B, F, ...] (a CPU tensor is staged chunk by chunk, stream ordered), or rg = (clips, counts, raw) of a
        ragged batch, every chunk packed [sum(counts), ...] with F its largest count."""
        step = self.max_batch
        if rg is None:
            for b0 in range(0, fr.shape[0], step):
                chunk = self._to_device(fr[b0:b0 + step])
                yield (b0,) + tuple(chunk.shape[:4]) + (chunk,)
        else:
            parts, counts, raw = rg
            for b0 in range(0, len(counts), step):
                chunk, cc = self._pack_to_device(parts[b0:b0 + step], raw), counts[b0:b0 + step]
                yield (b0, len(cc), max(cc)) + tuple(chunk.shape[1:3]) + (chunk,)

    def _draft_call(self, name, head, mid, draft, max_len, mode, ids, steps, lp=None, opts=None, tk=None) -> dict:
        """One of the two draft entry points (``head`` / ``mid`` = the arguments in front of the draft's / between the stop rule
        and ids_out); ``draft`` int64 [B, 1+n] on either device, trimmed to max_len columns beyond CLS.  -> what the call
        offered, accepted (summed over the clips) and decoded behind it; ``last_accepted`` = the clips' own numbers."""
        B = ids.shape[0]
        d = draft[:, :1 + max_len].to(self._dev).contiguous()
        n = d.shape[1] - 1
        acc = (ctypes.c_int32 * B)(*([-1] * B))
        before = self.draft_stats()
        (opts or _CallOptions(self)).attach(lp, tk)          # (tk: the call refuses it and consumes it)
        self._call(name, *head, _lib.ptr(d), n + 1, n, max_len, mode, *mid, _lib.ptr(ids), _lib.ptr(steps), acc, self._stream())
        after = self.draft_stats()
        self.last_accepted = torch.tensor(list(acc), dtype=torch.int32)
        return dict(draft_tokens=after[1] - before[1], accepted=after[2] - before[2], tail_steps=after[3] - before[3])

    def draft_stats(self):
        """gitcap_draft_stats: (draft calls, tokens offered, tokens accepted -- both summed over the clips --, tail steps)."""
        out = (ctypes.c_int64 * 4)()
        self._call("gitcap_draft_stats", out)
        return tuple(int(v) for v in out)

    def _greedy_decode(self, src, max_len, mode, want_lp=False, opts=None, rg=None, draft=None, want_att=False):
        """rg: the (clips, counts, raw) of a ragged batch (src is then unused): each chunk of at most max_batch clips is packed
        and runs with its counts attached.  draft: greedy_decode's (fp32 frames; camera frames are decoded by the plain call)."""
        self._drain()
        opts = opts or _CallOptions(self)
        if rg is None:
            fr, raw = self._check_frames(src)     # raw: camera frames [B,F,H,W,3] uint8 BGR, transform fused into the patch gather
        else:
            fr, raw, src = None, rg[2], rg[0][0]  # (src: where the results go)
        if draft is not None and raw:
            raise ValueError("draft= takes transformed fp32 frames (there is no draft form of the camera-frame call)")
        outs, steps_all, lps, accepted, tks, atts = [], [], [], [], [], []
        # (a batch of several chunks stops by the rule over the WHOLE batch, below: its chunks decode every step)
        dmode = mode if draft is None or (len(rg[1]) if rg is not None else fr.shape[0]) <= self.max_batch else STOP_NEVER
        with torch.cuda.device(self._dev):
            for b0, nb, F, fh, fw, chunk in self._chunks(fr, rg):
                ids = torch.empty((nb, max_len + 1), dtype=torch.int64, device=self._dev)
                steps = torch.zeros((1,), dtype=torch.int32, device=self._dev)
                if want_lp:
                    lps.append(torch.empty((nb, max_len), dtype=torch.float32, device=self._dev))
                tk = opts.topk_buffers(nb, max_len)
                if tk is not None:
                    tks.append(tk)
                if draft is not None:
                    self._draft_call("gitcap_greedy_draft", (_lib.ptr(chunk), nb, F), (), draft[b0:b0 + nb], max_len, dmode, ids, steps,
                                     lps[-1] if want_lp else None, opts.rows(b0, b0 + nb), tk)
                    accepted.append(self.last_accepted)
                    outs.append(ids)
                    steps_all.append(steps)
                    continue
                opts.rows(b0, b0 + nb).attach(lps[-1] if want_lp else None, tk)  # one-shot: consumed by the greedy call below
                if raw:
                    self._call("gitcap_greedy_raw", _lib.ptr(chunk), nb, F, fh, fw, max_len, mode,
                               _lib.ptr(ids), _lib.ptr(steps), self._stream())
                else:
                    self._call("gitcap_greedy", _lib.ptr(chunk), nb, F, max_len, mode, _lib.ptr(ids), _lib.ptr(steps),
                               self._stream())
                if want_att:        # the maps of the positions the loop just cached (include/gitcap.h: gitcap_attention_map)
                    fm = torch.empty((nb, max_len, F), dtype=torch.float32, device=self._dev)
                    tm = torch.empty((nb, max_len), dtype=torch.float32, device=self._dev)
                    self._call("gitcap_attention_map", nb, max_len, -1, None, _lib.ptr(fm), F, _lib.ptr(tm), None, 0, self._stream())
                    atts.append((fm, tm))
                outs.append(ids)
                steps_all.append(steps)
        self._last_memory = None
        if accepted:
            self.last_accepted = torch.cat(accepted)
        ids = torch.cat(outs, 0)
        if mode == STOP_ALL_SEP:
            if len(outs) == 1:
                n = int(steps_all[0].item())
            else:   # the rule is over the WHOLE batch: first step at which every row emitted SEP
                all_sep = (ids[:, 1:] == self.sep_token_id).all(dim=0)
                nz = torch.nonzero(all_sep)
                n = int(nz[0].item()) + 1 if nz.numel() else max_len
            ids = ids[:, :1 + n]
        mv = lambda t: t.to(src.device) if src.device != t.device else t
        out = (mv(ids),)
        if want_lp:
            out += (mv(torch.cat(lps, 0)[:, :ids.shape[1] - 1]),)
        if tks:
            out += tuple(mv(torch.cat([t[i] for t in tks], 0)[:, :ids.shape[1] - 1]) for i in (0, 1))
        if atts:
            Fm = max(a[0].shape[2] for a in atts)
            fm = torch.cat([a[0] if a[0].shape[2] == Fm else torch.nn.functional.pad(a[0], (0, Fm - a[0].shape[2])) for a in atts], 0)
            out += (mv(fm[:, :ids.shape[1] - 1]), mv(torch.cat([a[1] for a in atts], 0)[:, :ids.shape[1] - 1]))
        return out if len(out) > 1 else out[0]

    generate = greedy_decode      # the name BASELINE.json's north_star uses for this entry point

    @torch.no_grad()
    def greedy_decode_async(self, src: torch.Tensor, max_len: int = 10, stop: Optional[str] = None,
                            coalesce: int = 1, prompt=None, prompt_lengths=None, no_repeat_ngram_size: int = 0, min_length: int = 0,
                            suppress_tokens=None, frame_counts=None, top_logprobs: int = 0, return_attention: bool = False) -> "CaptionFuture":
        """Pipelined greedy_decode for a stream of batches: returns immediately with a future; up to
        FOUR submissions may be in flight, so one batch's image pass (MFMA bound) overlaps the token
        loops (latency bound) of the batches before it on the handle's internal HIP streams.  Call
        ``.result()`` (in submission order) to make the current stream wait and get the ids.

        `src` may be transformed fp32 frames [B,F,3,S,S] or uint8 BGR camera frames [B,F,H,W,3] (the transform of
        dataloader.py:18-32 then runs on the device, fused with the patch gather), on the device or -- what the reference's
        callers hold -- in HOST memory: a CPU tensor goes through a pinned staging ring (_StagingRing), so its host -> device
        copy runs under the compute of the batches before it (page-locked tensors, e.g. from DataLoader(pin_memory=True), are
        copied from where they are).  A CPU tensor must not be modified before ``result()``.

        ``coalesce=k`` (dynamic batching): k consecutive calls with the same shape are concatenated and
        run as ONE pass of k*B clips (the per-clip results are bitwise the same: the kernels are batch
        invariant); a ``result()`` on a batch that is still waiting for partners flushes it.  Needs
        max_batch >= k*B.  ``prompt`` / ``prompt_lengths`` as in greedy_decode; a prompted batch is submitted on its own (it does
        not coalesce).  no_repeat_ngram_size / min_length / suppress_tokens as in greedy_decode; a constrained batch coalesces
        only with batches that carry equal constraints.  frame_counts (or a list of clips) as in greedy_decode: a ragged batch is
        packed once (host clips: in the staging ring's pinned buffer) and submitted on its own (it does not coalesce).
        top_logprobs=k as in greedy_decode: ``result()`` returns (ids, top_ids, top_logprobs); batches coalesce with equal k."""
        if return_attention:
            raise ValueError("return_attention= is not taken by greedy_decode_async (its cache rows are not a caption's positions in order, or not the caller's to read yet): use attention(x, predictions) on the result")
        if not 0 <= int(top_logprobs) <= 32:
            raise ValueError(f"top_logprobs={top_logprobs} outside 0..32")
        stop = stop or self.stop
        mode = {"all_sep": STOP_ALL_SEP, "never": STOP_NEVER}[stop]
        if max_len > self.max_text_len:
            raise ValueError(f"max_len {max_len} > max_text_len={self.max_text_len} the handle was created for")
        if frame_counts is not None or not isinstance(src, torch.Tensor):
            src, rg = self._ragged_input(src, frame_counts)
            if rg is not None:                    # one submission of its own, the counts attached beside prompt and constraints
                parts, counts, raw = rg
                if len(counts) > self.max_batch:
                    raise ValueError(f"batch {len(counts)} > max_batch={self.max_batch}")
                self._flush_pending()
                opts = self._greedy_options(len(counts), max_len, prompt, prompt_lengths, no_repeat_ngram_size, min_length, suppress_tokens, rg)
                opts.top_k = int(top_logprobs)
                fut = CaptionFuture(self, None, mode, max_len, parts[0].device, opts)
                fut._attach(self._greedy_submit(self._ragged_source(rg), raw, (len(counts), max(counts)) + tuple(parts[0].shape[1:3]),
                                                max_len, mode, opts), 0, len(counts))
                return fut
        fr, raw = self._check_frames(src)         # nothing is copied yet: a CPU batch is staged when its group is submitted
        B = fr.shape[0]
        if B * max(1, coalesce) > self.max_batch:
            raise ValueError(f"batch {B} x coalesce {coalesce} > max_batch={self.max_batch}")
        host = fr.device.type == "cpu"
        if not host:
            fr = self._to_device(fr)
        opts = self._greedy_options(B, max_len, prompt, prompt_lengths, no_repeat_ngram_size, min_length, suppress_tokens)
        opts.top_k = int(top_logprobs)
        fut = CaptionFuture(self, fr, mode, max_len, src.device, opts)
        key = (tuple(fr.shape), max_len, mode, raw, host) + opts.key
        if opts.prompt is not None:
            coalesce = 1
        if self._pending and self._pending_key != key:
            self._flush_pending()
        self._pending.append(fut)
        self._pending_key = key
        if len(self._pending) >= max(1, coalesce):
            self._flush_pending()
        return fut

    def _ragged_source(self, rg):
        """The clips of a ragged batch as _submit_frames takes them: host clips as they are (packed by the staging ring), device
        clips packed."""
        parts, _, raw = rg
        return list(parts) if parts[0].device.type == "cpu" else self._pack_to_device(parts, raw)

    def _stage_group(self, parts, raw):
        """Host-fed submission: the callers' CPU tensors -> one ring entry (pinned staging unless the single tensor is already
        page-locked) -> device.  Returns (device frames, ring entry, the stream the copy is on = what the submission is ordered behind)."""
        dv, entry, st = self._staging().stage(self, parts, torch.uint8 if raw else torch.float32)
        return dv, entry, ctypes.c_void_p(st.cuda_stream)

    def _submit_frames(self, kind, src, raw, dims, args, outs, opts, users=1, before=None):
        """One pipelined submission, gitcap_<kind>[_raw]_submit (kind: "greedy" | "beam_search") -> its _Submission, in flight.
        src: the device frames (dense [B, F, ...] or packed), or the list of the callers' CPU tensors, which go through the staging
        ring (concatenated along dim 0) with the submission ordered behind their copy; dims = (B, F, fh, fw) as the call takes
        them; args: the call's arguments between the frame sizes and the stream; outs: the buffers it writes."""
        while len(self._inflight) >= 4:        # four slots: the oldest submission's slot is about to be reused (and, before the
            self._wait_submission(self._inflight[0])                       # staging, its ring entry)
        with torch.cuda.device(self._dev):
            parts = entry = None
            if isinstance(src, list):
                parts = src
                frames, entry, stream = self._stage_group(parts, raw)
            else:
                frames, stream = src, self._stream()
            ticket = ctypes.c_int(-1)
            self._submit(f"gitcap_{kind}_raw_submit" if raw else f"gitcap_{kind}_submit", _lib.ptr(frames), *(dims if raw else dims[:2]),
                         *args, stream, ctypes.byref(ticket), before=before or opts.attach)
        self._last_memory = None
        sub = _Submission(ticket.value, frames, outs, users > 1, users=users, parts=parts)
        if entry is not None:
            entry["sub"] = sub
        self._inflight.append(sub)
        return sub

    def _greedy_submit(self, src, raw, dims, max_len, stop, opts, users=1):
        ids = torch.empty((dims[0], max_len + 1), dtype=torch.int64, device=self._dev)
        steps = torch.zeros((1,), dtype=torch.int32, device=self._dev)
        tk = opts.topk_buffers(dims[0], max_len)          # held by the submission beside ids: the device writes them until the wait
        return self._submit_frames("greedy", src, raw, dims, (max_len, stop, _lib.ptr(ids), _lib.ptr(steps)), (ids, steps) + (tk or ()), opts,
                                   users, before=None if tk is None else (lambda: opts.attach(tk=tk)))

    def _flush_pending(self):
        """Submit the waiting batches as one pass and hand each future its row range."""
        group, self._pending = self._pending, []
        if not group:
            return
        raw, host = self._pending_key[3], self._pending_key[4]
        frames = [f._frames for f in group]
        dims = (sum(f.shape[0] for f in frames),) + tuple(frames[0].shape[1:4])
        if not host:
            frames = frames[0] if len(group) == 1 else torch.cat(frames, 0)
        stop = STOP_NEVER if len(group) > 1 else group[0]._mode     # the stop rule is per caller batch: applied in result()
        # the group's options are its first batch's: a prompted batch is a group of one, and every batch of a group carries equal
        # constraints (the key holds them)
        shared = self._greedy_submit(frames, raw, dims, group[0]._max_len, stop, group[0]._opts, users=len(group))
        r0 = 0
        for f in group:
            n = f._frames.shape[0]
            f._attach(shared, r0, r0 + n)
            r0 += n

    @torch.no_grad()
    def step_logits(self, ids_last: torch.Tensor, t: int, beams: int = 1) -> torch.Tensor:
        """One KV-cached decoding step = `scores = step(input_ids)` of model.py:519: ids_last [rows]
        is the token at text position t of every row; returns fp32 logits [rows, V]."""
        self._drain()
        ids = self._ids(ids_last).view(-1, 1)
        rows = ids.shape[0]
        logits = torch.empty((rows, self.cfg.vocab_size), dtype=torch.float32, device=self._dev)
        with torch.cuda.device(self._dev):
            self._call("gitcap_text_forward", _lib.ptr(ids), 1, rows, beams, t, 1, _lib.ptr(logits), 0, None, 0, self._stream())
        return logits

    @torch.no_grad()
    def infer(self, src: torch.Tensor, beam_size: int = 4, max_steps: int = 15, length_penalty: float = 0.6,
              per_node_beam_size: int = 2, num_keep_best: int = 1, save_logits: bool = False,
              on_device: Optional[bool] = None, repetition_penalty: float = 1.0, do_sample: bool = False, top_k: Optional[int] = None,
              top_p: Optional[float] = None, temperature: float = 1.0, seed: Optional[int] = None, prompt=None,
              prompt_lengths=None, no_repeat_ngram_size: int = 0, min_length: int = 0, suppress_tokens=None, frame_counts=None, return_attention: bool = False) -> dict:
        """GIT inference with beam search = ``GenerativeImageTextModel.infer`` (model.py:426-462) driven by
        ``GeneratorWithBeamSearchV2.search`` (model.py:479-678; defaults of :702-708).  Returns the
        reference's output dict: predictions [B, max_steps] (CLS-prefixed, EOS padded; [B, num_keep_best, max_steps] by descending
        score for num_keep_best > 1, the squeeze of :676), logprobs [B, num_keep_best] (-1e5 where a clip finished fewer),
        logits_dict (when save_logits, cf. :521: per-step [B*beams, V] host arrays from the host operator, which stops once every
        clip is done (:640); ONE device tensor [max_steps - 1, B*beams, V] from the device search, which runs every step) and
        visual_features.
        Default: the device-resident search (no host sync per step), whenever num_keep_best <= beam_size * per_node_beam_size
        <= 16 and per_node_beam_size >= 2; it keeps num_keep_best hypotheses and applies repetition_penalty (model.py:522-531) on
        the device (include/gitcap.h: gitcap_attach_search_options).  on_device=False runs the host-side operator of
        gitcap/search.py with the same two arguments (the default with save_logits).
        do_sample: the operator's sampling branch (model.py:532-554): temperature, top_k / top_p filter (at least 2 columns stay),
        per_node_beam_size draws per beam row instead of the best candidates.  On the device the draws come from a counter-based
        Philox stream keyed by `seed` (include/gitcap.h: gitcap_attach_sampling): the same seed, frames and batch position give the
        same caption from infer, infer_async and caption_stream; a clip's draws depend on its position in the batch.  seed=None
        takes one int64 from torch's global CPU generator (torch.manual_seed makes a run repeatable); the seed used is returned as
        ``seed``.  on_device=False draws with torch.multinomial from torch.Generator().manual_seed(seed): the two paths draw from
        different streams and agree in distribution only.
        prompt / prompt_lengths (as in greedy_decode): the `prefix` of model.py:432-437, one per clip and of any length below
        max_steps.  The search of a clip starts from its prompt; max_steps and the length penalty count the prompt's tokens, its
        tokens add nothing to a score, the repetition penalty sees them.  ``predictions`` INCLUDE each clip's prompt and the dict
        gains ``prompt_lengths`` [B] (CLS included), so a caller can strip what the reference strips at :455 -- the one deliberate
        difference: the reference returns predictions with its single prefix removed, which a ragged batch cannot do.
        on_device=False takes the reference's own route: the host operator clip by clip with start_predictions = the clip's prompt
        (the batch-of-one form of :436-437).
        no_repeat_ngram_size / min_length / suppress_tokens (as in greedy_decode): every beam row's banned columns are -inf before
        the step ranks or samples, ahead of the log-softmax (where the reference edits its logits, :522-531), so the scores
        renormalise over the allowed columns -- unlike HF's beam search, which masks after normalising.  min_length counts CLS and
        the prompt.  on_device=False applies the same rules in the host operator, on the raw logits next to its penalty.
        frame_counts (or ``src`` as a list of clips; as in greedy_decode): clips that differ in length.  The device search runs the
        batch packed, every clip's result bit for bit that of the clip alone; on_device=False runs the host operator clip by clip
        (the reference's teacher loop, model.py:765).  ``visual_features`` comes padded with ``visual_features_valid``."""
        if return_attention:
            raise ValueError("return_attention= is not taken by the beam family (infer) (its cache rows are not a caption's positions in order, or not the caller's to read yet): use attention(x, predictions) on the result")
        from .search import GeneratorWithBeamSearch
        if beam_size > self.max_beams:
            raise ValueError(f"beam_size {beam_size} > max_beams={self.max_beams} the handle was created for")
        if max_steps > self.max_text_len:
            raise ValueError(f"max_steps {max_steps} > max_text_len={self.max_text_len}")
        self._drain()
        rg = None
        if frame_counts is not None or not isinstance(src, torch.Tensor):
            src, rg = self._ragged_input(src, frame_counts)
        if rg is not None:
            parts, counts, raw = rg
            B = len(counts)
            if B > self.max_batch:
                raise ValueError(f"batch {B} > max_batch={self.max_batch}")
            if on_device is None:
                on_device = (not save_logits and 1 <= num_keep_best <= beam_size * per_node_beam_size <= 16
                             and per_node_beam_size >= 2)
            if not on_device:                    # the host operator, one clip at a time
                if prompt is not None:
                    raise ValueError("infer(on_device=False, frame_counts=...) takes no prompt")
                rs = [self.infer(p[None], beam_size, max_steps, length_penalty, per_node_beam_size, num_keep_best, save_logits, False,
                                 repetition_penalty, do_sample, top_k, top_p, temperature, seed, None, None, no_repeat_ngram_size,
                                 min_length, suppress_tokens) for p in parts]
                N = self.cfg.tokens_per_frame
                vis, valid = ragged.unpack_rows(torch.cat([r["visual_features"][0] for r in rs], 0), counts, N)
                return {"predictions": torch.cat([r["predictions"] for r in rs], 0), "logprobs": torch.cat([r["logprobs"] for r in rs], 0),
                        "logits_dict": [r["logits_dict"] for r in rs], "visual_features": vis, "visual_features_valid": valid}
            fr = self._pack_to_device(parts, raw)
        else:
            fr, raw = self._check_frames(src)
            B, F = fr.shape[:2]
            if B > self.max_batch:
                raise ValueError(f"batch {B} > max_batch={self.max_batch}")
            fr = self._to_device(fr)
        if on_device is None:
            on_device = (not save_logits and 1 <= num_keep_best <= beam_size * per_node_beam_size <= 16
                         and per_node_beam_size >= 2)
        sampling = self._seeded(self._sampling(do_sample, temperature, top_k, top_p, seed))
        pr = self._prompt(prompt, prompt_lengths, B, max_steps - 1, "max_steps - 1")
        co = self._constraints(no_repeat_ngram_size, min_length, suppress_tokens, max_steps, beam_size * per_node_beam_size)
        if on_device:
            self._check_device_search(beam_size, per_node_beam_size, num_keep_best, repetition_penalty, sampling)
            opts = _CallOptions(self, pr, co, None if rg is None else rg[1], num_keep_best, repetition_penalty, sampling)
            decoded, logprobs, steps, vis = self._infer_device(fr, opts, beam_size=beam_size, max_steps=max_steps, length_penalty=length_penalty,
                                                               per_node_beam_size=per_node_beam_size, sync=True,
                                                               save_logits=save_logits, want_visual=False, raw=raw)
            out = {"predictions": decoded, "logprobs": _lp2d(logprobs), "logits_dict": [] if steps is None else steps,
                   "visual_features": None}
            if sampling is not None:
                out["seed"] = sampling[3]
            if pr is not None:
                out["prompt_lengths"] = pr.lengths
            return out
        searcher = GeneratorWithBeamSearch(self.sep_token_id, max_steps, beam_size, per_node_beam_size, length_penalty,
                                           repetition_penalty=repetition_penalty, temperature=temperature,
                                           no_repeat_ngram_size=no_repeat_ngram_size, min_length=min_length,
                                           suppress_tokens=suppress_tokens)
        if pr is not None:
            return self._infer_host_prompted(fr, pr, searcher, beam_size, num_keep_best, save_logits, sampling, top_k, top_p)
        _, vis = self.forward_image_enc(fr)
        start = torch.full((B, 1), self.cls_token_id, dtype=torch.long, device=self._dev)      # model.py:429-431

        def step(ids):                       # decoding_step bound at model.py:442-445, KV-cached
            return self.step_logits(ids[:, -1], ids.shape[1] - 1, beams=beam_size)

        def reorder(beam_idx, cur_len):      # what model.py:623-634 leaves commented out
            self.reorder_rows(beam_idx, cur_len)

        if sampling is None:
            decoded, logprobs, saved = searcher.search(start, step, num_keep_best=num_keep_best, reorder=reorder,
                                                       save_logits=save_logits)
            return {"predictions": decoded, "logprobs": logprobs, "logits_dict": saved, "visual_features": vis}
        decoded, logprobs, saved = searcher.search(start, step, num_keep_best=num_keep_best, reorder=reorder, save_logits=save_logits,
                                                   do_sample=True, top_k=top_k, top_p=top_p,
                                                   generator=torch.Generator().manual_seed(sampling[3]))
        return {"predictions": decoded, "logprobs": logprobs, "logits_dict": saved, "visual_features": vis, "seed": sampling[3]}

    def _infer_host_prompted(self, fr, pr, searcher, beam_size, num_keep_best, save_logits, sampling, top_k, top_p):
        """infer(on_device=False, prompt=...): the host operator clip by clip from start_predictions = the clip's prompt.  The first
        step of a clip runs the whole prompt through the decoder (every beam row holds it); the steps behind it are KV-cached."""
        preds, lps, saved_all, vis_all = [], [], [], []
        for b in range(fr.shape[0]):
            _, vis = self.forward_image_enc(fr[b:b + 1])
            n = pr.host_lengths[b]
            start = pr.ids[b:b + 1, :n]

            def step(ids, n=n):
                if ids.shape[1] > n:
                    return self.step_logits(ids[:, -1], ids.shape[1] - 1, beams=beam_size)
                ids = self._ids(ids)
                logits = torch.empty((ids.shape[0], self.cfg.vocab_size), dtype=torch.float32, device=self._dev)
                with torch.cuda.device(self._dev):
                    self._call("gitcap_text_forward", _lib.ptr(ids), ids.shape[1], ids.shape[0], beam_size, 0, ids.shape[1], _lib.ptr(logits),
                               0, None, 0, self._stream())
                return logits

            kw = {} if sampling is None else dict(do_sample=True, top_k=top_k, top_p=top_p,
                                                  generator=torch.Generator().manual_seed(sampling[3]))
            decoded, logprobs, saved = searcher.search(start, step, num_keep_best=num_keep_best, reorder=self.reorder_rows,
                                                       save_logits=save_logits, **kw)
            preds.append(decoded); lps.append(logprobs); saved_all.append(saved); vis_all.append(vis)
        out = {"predictions": torch.cat(preds, 0), "logprobs": torch.cat(lps, 0), "logits_dict": saved_all,
               "visual_features": torch.cat(vis_all, 0), "prompt_lengths": pr.lengths}
        if sampling is not None:
            out["seed"] = sampling[3]
        return out

    @staticmethod
    def _sampling(do_sample, temperature, top_k, top_p, seed):
        """The sampling arguments of the public calls -> None (no sampling) or (temperature, top_k, top_p, seed | None)."""
        if not do_sample:
            return None
        return (float(temperature), int(top_k or 0), 1.0 if top_p is None else float(top_p), None if seed is None else int(seed))

    @staticmethod
    def _seeded(sampling):
        """A _sampling tuple with its seed filled in: None takes one int64 from torch's global CPU generator."""
        if sampling is None or sampling[3] is not None:
            return sampling
        return sampling[:3] + (int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item()),)

    def _check_device_search(self, beam_size, per_node_beam_size, num_keep_best=1, repetition_penalty=1.0, sampling=None):
        if per_node_beam_size < 2:
            raise ValueError("the device-resident search needs per_node_beam_size >= 2: with one candidate per beam "
                             "a single EOS leaves fewer than beam_size live beams (model.py:606 asserts against it); "
                             "the host operator (on_device=False) raises when that happens")
        if beam_size * per_node_beam_size > 16:
            raise ValueError("the device-resident search ranks at most 16 candidates per clip")
        if not 1 <= num_keep_best <= beam_size * per_node_beam_size:
            raise ValueError(f"num_keep_best {num_keep_best} outside [1, beam_size * per_node_beam_size = "
                             f"{beam_size * per_node_beam_size}]: a step ranks no more candidates than that")
        if not (math.isfinite(repetition_penalty) and repetition_penalty > 0):
            raise ValueError(f"repetition_penalty must be finite and > 0, got {repetition_penalty}")
        if sampling is not None:
            t, k, p = sampling[:3]
            if not (math.isfinite(t) and t > 0):
                raise ValueError("attach_sampling: temperature must be finite and > 0")
            if k < 0:
                raise ValueError("attach_sampling: top_k must be >= 0")
            if not 0 < p <= 1:
                raise ValueError("attach_sampling: top_p outside (0, 1]")
            if self.cfg.vocab_size > 32768:
                raise ValueError("beam_search: sampling takes a vocabulary of at most 32768 columns")
            if (p < 1 and per_node_beam_size > 2) or (k > 0 and max(k, 2) < per_node_beam_size):
                raise ValueError("beam_search: per_node_beam_size exceeds the columns the attached sampling filter is sure to keep")

    def _infer_device(self, src, opts, *, beam_size, max_steps, length_penalty, per_node_beam_size, sync, save_logits, want_visual,
                      raw=None, dims=None):
        """The device-resident search with the options `opts` (_CallOptions): synchronously on the current stream (sync=True; src =
        frames on the device, fp32 NCHW or raw uint8 HWC, packed for a ragged batch; per-step logits are not available from the
        synchronous entry point, so a call that wants them submits and waits) or as a pipelined submission (src and dims as
        _submit_frames takes them).  Returns (decoded, logprobs, step logits | None, visual | None), or when submitted the
        _Submission that holds them as its outs; with num_keep_best > 1 decoded is [B, n, max_steps] and logprobs [B, n]."""
        counts = opts.counts
        if raw is None:
            raw = src.dtype == torch.uint8
        if dims is None:                         # (a ragged batch: src holds the packed frames [sum(counts), ...], visual rows come packed)
            dims = tuple(src.shape[:4]) if counts is None else (len(counts), max(counts)) + tuple(src.shape[1:3])
        B, F = dims[:2]
        own, decoded, logprobs = opts.search_outputs(B, max_steps)      # own: the call's outputs, rank 0 of the n-best
        with torch.cuda.device(self._dev):
            if sync and not save_logits and not want_visual and not raw:
                self._drain()
                opts.attach()
                self._call("gitcap_beam_search", _lib.ptr(src), B, F, beam_size, max_steps, ctypes.c_float(length_penalty),
                           per_node_beam_size, _lib.ptr(own[0]), _lib.ptr(own[1]), self._stream())
                self._last_memory = None
                return decoded, logprobs, None, None
            steps = torch.empty((max_steps - 1, B * beam_size, self.cfg.vocab_size), dtype=torch.float32, device=self._dev) if save_logits else None
            vis_shape = (B, F * self.cfg.tokens_per_frame) if counts is None else (sum(counts) * self.cfg.tokens_per_frame,)
            vis = torch.empty(vis_shape + (self.cfg.enc_width,), dtype=torch.float32, device=self._dev) if want_visual else None
        args = (_lib.ptr(vis), beam_size, max_steps, ctypes.c_float(length_penalty), per_node_beam_size, _lib.ptr(own[0]), _lib.ptr(own[1]),
                _lib.ptr(steps))
        sub = self._submit_frames("beam_search", src, raw, dims, args, (decoded, logprobs, steps, vis), opts)
        if not sync:
            return sub
        try:                                     # (a re-run, or a synchronous call that wants logits / visual features / takes raw frames)
            with torch.cuda.device(self._dev):
                self._call("gitcap_beam_search_wait", sub.ticket, self._stream())
        finally:
            self._inflight.remove(sub)           # waited for here: no future holds it
        return sub.outs

    @torch.no_grad()
    def infer_async(self, src: torch.Tensor, beam_size: int = 4, max_steps: int = 15, length_penalty: float = 0.6,
                    per_node_beam_size: int = 2, save_logits: bool = False, visual_features: bool = False,
                    num_keep_best: int = 1, repetition_penalty: float = 1.0, do_sample: bool = False, top_k: Optional[int] = None,
                    top_p: Optional[float] = None, temperature: float = 1.0, seed: Optional[int] = None, prompt=None,
                    prompt_lengths=None, no_repeat_ngram_size: int = 0, min_length: int = 0, suppress_tokens=None,
                    frame_counts=None, return_attention: bool = False) -> "InferFuture":
        """Pipelined ``infer`` (the device-resident search) for a stream of batches: returns at once with a future; up to FOUR
        submissions (of this kind or of greedy_decode_async) may be in flight, so one batch's image pass overlaps the search loops
        of the batches before it.  ``result()`` returns ``infer``'s dict; with ``save_logits`` its ``logits_dict`` is one device
        tensor [max_steps - 1, B * beam_size, V] (the raw logits of every step, model.py:521), with ``visual_features`` the fp32
        features [B, F*N, Dv] (model.py:460); num_keep_best / repetition_penalty as in ``infer``.  Results are bitwise those of the
        synchronous call, with do_sample too (its arguments as in ``infer``; the seed is fixed at submission and returned as
        ``seed``) and with prompt / prompt_lengths (as in ``infer``; the dict gains ``prompt_lengths``) and with no_repeat_ngram_size / min_length / suppress_tokens (as in ``infer``).
        `src` as in greedy_decode_async: fp32 frames or uint8 camera frames, on the device or in host memory (staged through the pinned ring)."""
        if return_attention:
            raise ValueError("return_attention= is not taken by the beam family (infer_async) (its cache rows are not a caption's positions in order, or not the caller's to read yet): use attention(x, predictions) on the result")
        sampling = self._seeded(self._sampling(do_sample, temperature, top_k, top_p, seed))
        self._check_device_search(beam_size, per_node_beam_size, num_keep_best, repetition_penalty, sampling)
        if beam_size > self.max_beams:
            raise ValueError(f"beam_size {beam_size} > max_beams={self.max_beams} the handle was created for")
        if max_steps > self.max_text_len:
            raise ValueError(f"max_steps {max_steps} > max_text_len={self.max_text_len}")
        if self._pending:
            self._flush_pending()
        rg = None
        if frame_counts is not None or not isinstance(src, torch.Tensor):
            src, rg = self._ragged_input(src, frame_counts)
        if rg is not None:                       # packed once (host clips in the staging ring), submitted with its counts attached
            parts, counts, raw = rg
            B, out_device, dims = len(counts), parts[0].device, (len(counts), max(counts)) + tuple(parts[0].shape[1:3])
        else:
            fr, raw = self._check_frames(src)
            B, out_device, counts, dims = fr.shape[0], src.device, None, tuple(fr.shape[:4])
        if B > self.max_batch:
            raise ValueError(f"batch {B} > max_batch={self.max_batch}")
        opts = _CallOptions(self, self._prompt(prompt, prompt_lengths, B, max_steps - 1, "max_steps - 1"),
                            self._constraints(no_repeat_ngram_size, min_length, suppress_tokens, max_steps, beam_size * per_node_beam_size),
                            counts, num_keep_best, repetition_penalty, sampling)
        if rg is not None:
            fr = self._ragged_source(rg)
        else:
            fr = [fr] if fr.device.type == "cpu" else self._to_device(fr)
        search = dict(beam_size=beam_size, max_steps=max_steps, length_penalty=length_penalty, per_node_beam_size=per_node_beam_size)
        sub = self._infer_device(fr, opts, sync=False, save_logits=save_logits, want_visual=visual_features, raw=raw, dims=dims, **search)
        return InferFuture(self, sub, opts, search, out_device, save_logits)

    def caption_stream(self, batch: int = 1, window: Optional[int] = None, hop: int = 1, max_len: int = 20, stop: Optional[str] = None,
                       beam_size: Optional[int] = None, length_penalty: float = 0.6, per_node_beam_size: Optional[int] = None,
                       visual_features: bool = False, gate=None, logprobs: bool = False, num_keep_best: int = 1,
                       repetition_penalty: float = 1.0, do_sample: bool = False, top_k: Optional[int] = None,
                       top_p: Optional[float] = None, temperature: float = 1.0, seed: Optional[int] = None, prompt=None,
                       prompt_lengths=None, no_repeat_ngram_size: int = 0, min_length: int = 0, suppress_tokens=None,
                       carry: bool = False, top_logprobs: int = 0, return_attention: bool = False) -> CaptionStream:
        """A sliding caption window over live frames (the reference's real-time loop): ``push(frames)`` appends
        frames of `batch` clips and returns the caption of the last `window` frames (default: the model's num_frames) once the
        window is full and `hop` frames have arrived since the last one, else None.  Each frame is encoded once.  Greedy by
        default (ids as greedy_decode(max_len, stop)); with beam_size the dict of infer's device search (max_len = its
        max_steps; visual_features adds the window's features; num_keep_best / repetition_penalty as in infer).  One live stream per model: opening another one, or .to() /
        .cuda(), invalidates this one.  ``gate``: a gitcap.framegate.FrameGate that decides on the device which pushed camera frames
        are worth encoding (it is reset here); without one every pushed frame is.  ``logprobs`` (greedy streams only): after a push
        that returned a caption, ``stream.last_logprobs`` holds its per-token log-probabilities [B, steps] (greedy_decode's
        return_logprobs; gitcap.caption_confidence turns them into one number per clip).  do_sample / top_k / top_p / temperature /
        seed (beam streams only) as in infer: every caption samples with `seed` (seed=None: a fresh one per caption from torch's
        global CPU generator); ``stream.last_seed`` is the seed of the caption the last push returned.  prompt / prompt_lengths (as
        in greedy_decode / infer): the stream's prompt, one row per clip, attached again for every caption.  no_repeat_ngram_size /
        min_length / suppress_tokens (as in greedy_decode / infer): the stream's constraints, attached again for every caption.
        ``carry`` (greedy streams without prompt or constraints): the previous caption is the draft of the next window call
        (greedy_decode's ``draft``): the same captions; ``stream.stats()`` tells how much of the drafts was accepted.
        ``top_logprobs=k`` (greedy streams without ``carry``): ``stream.last_top_ids`` / ``stream.last_top_logprobs`` [B, steps, k]
        of the caption the last push returned (greedy_decode's top_logprobs)."""
        if return_attention:
            raise ValueError("return_attention= is not taken by the window streams (caption_stream) (its cache rows are not a caption's positions in order, or not the caller's to read yet): use attention(x, predictions) on the result")
        if not 0 <= int(top_logprobs) <= 32:
            raise ValueError(f"top_logprobs={top_logprobs} outside 0..32")
        if top_logprobs and (beam_size is not None or carry):
            raise ValueError("top_logprobs is for greedy streams without carry (a draft call does not carry alternatives)")
        if carry and beam_size is not None:
            raise ValueError("carry=True is for greedy streams (beam_size=None)")
        if carry and (prompt is not None or no_repeat_ngram_size or min_length or suppress_tokens is not None):
            raise ValueError("carry=True is not combined with prompt= or the constraint arguments")
        if logprobs and beam_size is not None:
            raise ValueError("logprobs=True is for greedy streams (the beam-search dict carries its own sequence score)")
        window = int(window or max(1, self.cfg.num_frames))
        if batch > self.max_batch or window > self.max_frames or (self.cfg.num_frames > 0 and window > self.cfg.num_frames):
            raise ValueError(f"batch {batch} / window {window} exceed max_batch={self.max_batch} / max_frames={self.max_frames} "
                             f"/ num_frames={self.cfg.num_frames}")
        if max_len > self.max_text_len:
            raise ValueError(f"max_len {max_len} > max_text_len={self.max_text_len} the handle was created for")
        mode = {"all_sep": STOP_ALL_SEP, "never": STOP_NEVER}[stop or self.stop]
        sampling = self._sampling(do_sample, temperature, top_k, top_p, seed)
        if beam_size is None:
            if visual_features:
                raise ValueError("visual_features come with the beam-search dict (beam_size=...)")
            if num_keep_best != 1 or repetition_penalty != 1.0:
                raise ValueError("num_keep_best / repetition_penalty are options of the beam search (beam_size=...)")
            if do_sample:
                raise ValueError("do_sample is an option of the beam search (beam_size=...)")
        else:
            per_node_beam_size = 2 if per_node_beam_size is None else per_node_beam_size
            self._check_device_search(beam_size, per_node_beam_size, num_keep_best, repetition_penalty, sampling)
            if beam_size > self.max_beams:
                raise ValueError(f"beam_size {beam_size} > max_beams={self.max_beams} the handle was created for")
        if gate is not None:
            if not isinstance(gate, FrameGate):
                raise ValueError(f"gate must be a gitcap.framegate.FrameGate, got {type(gate).__name__}")
            gate.reset()
        pr = self._prompt(prompt, prompt_lengths, batch, max_len if beam_size is None else max_len - 1,
                          "max_len" if beam_size is None else "max_len - 1")
        co = self._constraints(no_repeat_ngram_size, min_length, suppress_tokens, max_len,
                               1 if beam_size is None else beam_size * per_node_beam_size)
        return CaptionStream(self, batch, window, hop, max_len, mode, beam_size, length_penalty, per_node_beam_size, visual_features, gate,
                             logprobs, num_keep_best, repetition_penalty,
                             sampling, pr, co, carry, top_logprobs)

    def stream_pool(self, streams: int, frames: Optional[int] = None, hop: int = 1, min_frames: int = 1, max_len: int = 20,
                    stop: Optional[str] = None, beam_size: Optional[int] = None, logprobs: bool = False, top_logprobs: int = 0,
                    prompt=None, no_repeat_ngram_size: int = 0, min_length: int = 0, suppress_tokens=None,
                    length_penalty: float = 0.6, per_node_beam_size: int = 2) -> TeacherStreamPool:
        """Several live cameras on one model (the multi-camera loop): `streams` independent windows of `frames`
        frames (default: the model's num_frames).  ``pool.push(frames, streams)`` takes n frames for any streams in any mix (frame i
        belongs to stream streams[i]) -- uint8 camera frames [n,H,W,3] or transformed fp32 frames [n,3,S,S], on the host or the
        device --, encodes them once in one packed pass and returns ``{stream: ids}`` for every stream that is due: at least `hop`
        of its frames have arrived since its last caption and it holds at least `min_frames` frames (1: a caption from a camera's
        first frame on; `frames`: only full windows).  The due streams are captioned as one ragged batch, in chunks of max_batch
        (include/gitcap.h: gitcap_pool_*).  A stream's caption is bit for bit greedy_decode(max_len, stop) on a list holding that
        stream's last frames, cut behind the row's own first SEP under the all_sep rule (not at the batch-wide step count): it
        does not depend on which other streams were due.  ``logprobs`` / ``top_logprobs=k``: ``pool.last_logprobs[stream]``,
        ``pool.last_top_ids[stream]`` / ``pool.last_top_logprobs[stream]`` of a stream's latest caption, cut the same way;
        ``pool.last_frames[stream]`` = the frames it saw.  ``beam_size=k`` (with length_penalty / per_node_beam_size as in infer):
        a caption is the device search's best hypothesis [max_len] (max_len = infer's max_steps; EOS padded, not cut) and
        ``pool.last_scores[stream]`` its score, bit for bit infer on a one-clip list of the stream's frames.  prompt (one row of
        token ids: every stream's captions start from it) and no_repeat_ngram_size / min_length / suppress_tokens (as in
        greedy_decode / infer) hold for every stream and are attached again for every pool call; per-camera prompts or rules are
        not part of the pool.  ``pool.caption(streams)`` captions now, ``pool.drop(stream)`` empties one stream,
        ``pool.counts()`` = frames held per stream.
        The pool and a caption_stream() of the same model live side by side: opening one does not invalidate the other.  Opening
        another pool, moving the model or loading weights invalidates this one.
        Out of scope: scene-change gates (put one FrameGate per camera in front of ``push``), ``carry`` / drafts, visual
        features and attention maps, pipelined submission."""
        if not 0 <= int(top_logprobs) <= 32:
            raise ValueError(f"top_logprobs={top_logprobs} outside 0..32")
        if streams < 1 or streams > 4096:
            raise ValueError(f"streams={streams} outside 1..4096")
        window = int(frames or max(1, self.cfg.num_frames))
        if window < 1 or window > self._frame_limit():
            raise ValueError(f"frames={window} outside 1..{self._frame_limit()} (max_frames / num_frames)")
        if max_len < 1 or max_len > self.max_text_len:
            raise ValueError(f"max_len={max_len} outside 1..max_text_len={self.max_text_len}")
        mode = {"all_sep": STOP_ALL_SEP, "never": STOP_NEVER}[stop or self.stop]
        beam = None
        if beam_size is not None:
            if logprobs or top_logprobs:
                raise ValueError("logprobs / top_logprobs are for greedy pools (a search carries its own sequence score)")
            self._check_device_search(beam_size, per_node_beam_size)
            if beam_size > self.max_beams:
                raise ValueError(f"beam_size {beam_size} > max_beams={self.max_beams} the handle was created for")
            if max_len < 2:
                raise ValueError("a search takes max_len >= 2")
            beam = (int(beam_size), float(length_penalty), int(per_node_beam_size))
        pr = None
        if prompt is not None:          # one row for every stream: max_batch copies, a pool call attaches the rows it needs
            row = torch.as_tensor(prompt).detach().to("cpu", torch.int64).reshape(-1)
            pr = self._prompt([row] * self.max_batch, None, self.max_batch, max_len if beam is None else max_len - 1,
                              "max_len" if beam is None else "max_len - 1")
        co = self._constraints(no_repeat_ngram_size, min_length, suppress_tokens, max_len, 1 if beam is None else beam[0] * beam[2])
        return TeacherStreamPool(self, streams, window, hop, max_len, mode, logprobs, top_logprobs, min_frames, (pr, co), beam)

    def beam_search(self, src: torch.Tensor, max_len: int = 10, k: int = 3) -> torch.Tensor:
        """Signature of StudentCandidateV1.beam_search (model.py:189): best sequence per clip
        [B, max_len], found with the GIT search operator (length penalty 0.6, model.py:702-708)."""
        out = self.infer(src, beam_size=k, max_steps=max_len)["predictions"]
        return out.to(src.device) if src.device != out.device else out

    def reorder_rows(self, src_rows: torch.Tensor, t_len: int):
        """Beam reorder of the text K/V cache (what model.py:623-634 sketches in comments)."""
        idx = src_rows.to(device=self._dev, dtype=torch.int32).contiguous()
        with torch.cuda.device(self._dev):
            self._call("gitcap_reorder_rows", _lib.ptr(idx), idx.numel(), t_len, self._stream())

    PROF_CLASSES = ("gemm", "attn_full", "skinny", "attn_text", "rowops", "gemm_ln")

    def profile(self, enable: bool):
        self._call("gitcap_profile_enable", int(bool(enable)))

    def profile_read(self) -> dict:
        """{class: {ms, launches, flops, bytes}} summed over the bracketed launches since the last read."""
        out = {}
        for i, name in enumerate(self.PROF_CLASSES):
            ms, fl, by = ctypes.c_double(), ctypes.c_double(), ctypes.c_double()
            n = ctypes.c_int64()
            self._call("gitcap_profile_read", i, ctypes.byref(ms), ctypes.byref(n), ctypes.byref(fl), ctypes.byref(by))
            out[name] = dict(ms=ms.value, launches=n.value, flops=fl.value, bytes=by.value)
        return out

    def set_fp8_scale(self, scale: float):
        """Static power-of-two scale of the e4m3 activation codes of compute='fp8_ffn' (gitcap_set_fp8_scale): codes hold
        value / scale and reach +-448.  Synchronises the device."""
        self._drain()
        self._call("gitcap_set_fp8_scale", ctypes.c_float(float(scale)))
        self.fp8_scale = float(scale)
        self._kw["fp8_scale"] = self.fp8_scale
        self._last_memory = None

    def fp8_saturations(self, reset: bool = True) -> int:
        """Activation codes of valid image rows that compute='fp8_ffn' clamped at +-448 since the last reset
        (gitcap_fp8_saturations).  0 for any other compute mode.  Synchronises the device."""
        n = ctypes.c_int64()
        self._call("gitcap_fp8_saturations", ctypes.byref(n), int(bool(reset)))
        return n.value

    def weight_bytes(self) -> int:
        """Device bytes of the loaded tensors (GEMM weights + scales, tables, biases)."""
        n = ctypes.c_int64()
        self._lib.gitcap_weight_bytes(self._handle, ctypes.byref(n))
        return n.value

    def workspace_bytes(self) -> int:
        n = ctypes.c_int64()
        self._lib.gitcap_workspace_bytes(self._handle, ctypes.byref(n))
        return n.value


@torch.no_grad()
def draft_and_verify(teacher: GitCaptioner, student, src: torch.Tensor, max_len: int = 20, student_src: Optional[torch.Tensor] = None,
                     **greedy_kw) -> dict:
    """Student drafts, teacher verifies: the student (a StudentCaptioner) captions ``src`` -- or ``student_src`` where its input
    differs from the teacher's: frames of its encoder's size, or memory tokens [B, F, d_model] -- and the teacher's
    greedy_decode(src, max_len, draft=that caption, **greedy_kw) verifies it.  -> dict(ids, draft, accepted[, logprobs]): ``ids``
    (and ``logprobs`` with return_logprobs=True) are bit for bit the teacher's plain greedy_decode whatever the student wrote,
    ``draft`` the student's caption, ``accepted`` int32 [B] the leading draft tokens the teacher kept per clip.
    Clips that differ in length (``src`` / ``student_src`` as lists of clips, or padded with ``frame_counts=``) go to both models
    as they are; a clip has at most min(the teacher's frame limit, the student's mem_tokens) frames."""
    fc = {} if greedy_kw.get("frame_counts") is None else {"frame_counts": greedy_kw["frame_counts"]}
    draft = student.greedy_decode(src if student_src is None else student_src, max_len=min(max_len, student.max_text_len), stop="never", **fc)
    out = teacher.greedy_decode(src, max_len=max_len, draft=draft, **greedy_kw)
    ids, lp = out if isinstance(out, tuple) else (out, None)
    res = dict(ids=ids, draft=draft, accepted=teacher.last_accepted)
    if lp is not None:
        res["logprobs"] = lp
    return res
