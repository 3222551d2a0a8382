"""``StudentCaptioner``: the reference's ``StudentCandidateV1`` call surface
(/root/reference/src/models/model.py:50-187) over libgitcap's student-decoder entry points
(include/gitcap.h, csrc/student.hip).  SURVEY.md par. 8 row f.2.

Same constructor keywords (model.py:55-57), ``forward`` / ``forward_image_enc`` /
``forward_decoder`` / ``greedy_decode`` with the reference's argument meaning, ``state_dict`` keys of
the reference.  The decoder (embedding, positional table, 2 x (self-attention, cross-attention over the
frame tokens, FFN), vocabulary head, greedy loop with the all-rows-SEP stop rule) runs in HIP kernels
with an exact KV cache.  The TinyViT image encoder runs on the HIP kernels of csrc/tinyvit.hip
(``gitcap.tinyvit.TinyViTEncoder``): ``image_encoder="native"`` builds it from ``image_enc_name``, or the caller
passes a ``TinyViTEncoder``; then frames ``[B,F,3,H,W]`` go to a caption on the device, the encoder's memory never
leaving it.  Any other module mapping ``[B*F,3,H,W]`` to the list of feature maps (model.py:117) is still accepted as
``image_encoder``; ``greedy_decode`` also accepts the frame features ``memory [B, F, d_model]`` directly.  With the
native encoder every frame argument may also be uint8 BGR camera frames ``[B,F,H,W,3]`` (what the reference's webcam loop
holds, src/real_time_inference.py:39), and ``caption_stream()`` captions a sliding window of live frames, encoding each
frame once (``StudentCaptionStream``).  There is no CPU or PyTorch fallback for the decoder or the native encoder.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Mapping, Optional

import numpy as np
import torch

from . import _lib, ragged
from ._handle import _NativeModule
from ._stream import STOP_ALL_SEP, STOP_NEVER, _WindowStream
from .framegate import FrameGate
from .streampool import StudentStreamPool
from .student_config import (CStudentConfig, StudentConfig, check_student_shapes, positional_table, student_shapes)
from .tinyvit import TinyViTEncoder, tinyvit_config
from .window import WindowSchedule

ENC_PREFIX = "image_encoder.model."


class _StudentConstraints:
    """Hard constraints of a student decoding call (include/gitcap.h: gitcap_student_attach_constraints): the n-gram size, the
    minimum length and the suppress list as a device int32 tensor (read by the consuming call, on its stream)."""

    def __init__(self, model, n, min_length, suppress):
        self.n, self.min_length, self.suppress = n, min_length, tuple(suppress)
        self._ids = torch.tensor(suppress, dtype=torch.int32, device=model._dev) if suppress else None
        self._c = _lib.CConstraints(n, min_length, None if self._ids is None else self._ids.data_ptr(), len(suppress))

    def attach(self, model):
        """The one-shot attachment the NEXT greedy- or beam-family call consumes (a repeated call attaches again)."""
        model._call("gitcap_student_attach_constraints", ctypes.byref(self._c))


class _StudentSearch:
    """The options of a beam-family call that ends hypotheses at SEP (include/gitcap.h: gitcap_student_attach_search), checked as the
    library checks them, before anything is launched.  ``run`` allocates the outputs, attaches and makes the call."""

    def __init__(self, k, length_penalty, num_keep_best, per_node_beam_size, repetition_penalty):
        pn = k if per_node_beam_size is None else int(per_node_beam_size)
        n = int(num_keep_best)
        if not 1 <= n <= k:
            raise ValueError(f"num_keep_best={num_keep_best} outside 1..k={k}")
        if not 2 <= pn <= k or k * pn > 16:
            raise ValueError(f"per_node_beam_size={pn} must be in 2..k={k} with k * per_node_beam_size <= 16 (eos=True needs k >= 2)")
        rp, lp = float(repetition_penalty), float(length_penalty)
        if not (rp > 0 and np.isfinite(rp) and np.isfinite(lp)):
            raise ValueError("repetition_penalty must be > 0 and finite, length_penalty finite")
        self.k, self.n, self.pn, self.rp, self.lp = int(k), n, pn, rp, lp

    def run(self, model, B, max_len, call) -> dict:
        """``call(ids_ptr)`` makes the library call that consumes the attachment -> predictions [B, n, max_len], scores and
        lengths [B, n], on the device."""
        dev = model._dev
        pred = torch.empty((B, self.n, max_len), dtype=torch.int64, device=dev)
        scores = torch.empty((B, self.n), dtype=torch.float32, device=dev)
        lengths = torch.empty((B, self.n), dtype=torch.int32, device=dev)
        c = _lib.CStudentSearchOptions(self.n, self.lp, self.pn, self.rp, scores.data_ptr(), lengths.data_ptr())
        model._call("gitcap_student_attach_search", ctypes.byref(c))
        call(_lib.ptr(pred))
        return dict(predictions=pred, scores=scores, lengths=lengths)


def _search_options(eos, k, length_penalty, num_keep_best, per_node_beam_size, repetition_penalty):
    """The search arguments of the beam-family calls -> _StudentSearch, or None for today's search (eos=False and the defaults)."""
    if eos:
        return _StudentSearch(k, length_penalty, num_keep_best, per_node_beam_size, repetition_penalty)
    if length_penalty != 1.0 or num_keep_best != 1 or per_node_beam_size is not None or repetition_penalty != 1.0:
        raise ValueError("length_penalty, num_keep_best, per_node_beam_size and repetition_penalty belong to the search that ends "
                         "hypotheses at SEP: pass eos=True")
    return None


def _constrained(no_repeat_ngram_size, min_length, suppress_tokens) -> bool:
    return bool(no_repeat_ngram_size or min_length or suppress_tokens is not None)


class StudentCaptionStream(_WindowStream):
    """Live captioning on the student over a sliding window of ``mem_tokens`` frames (StudentCaptioner.caption_stream;
    include/gitcap.h: gitcap_student_window_*).  A frame is encoded once, when it is pushed, and its cross-attention K|V rows
    are computed then; a caption of the window only orders those rows and runs the token loop.  Captions are bitwise those of
    greedy_decode / beam_search on the window's frames.  With a ``gate`` (gitcap.framegate.FrameGate) only the frames it admits
    are encoded and counted; a push of camera frames with none admitted returns None and costs one distance launch.  With
    ``carry`` a greedy stream offers its previous caption as the draft of the next window call
    (gitcap_student_window_greedy_draft): same captions, and a caption that repeats costs one pass instead of a token loop.
    ``constraints`` (a _StudentConstraints or None): the stream's hard constraints, attached again for every caption.
    ``prompt`` (caption_stream's ``prompt=``, or None): one text prefix per stream row, attached again for every caption; the
    ``prompt`` property replaces it (None: no prompt from the next caption on) and ``prompt_lengths`` [batch] tells how many leading
    tokens of every caption row are the prompt's (CLS included; None without a prompt).
    ``search`` (a _StudentSearch or None; streams with ``beams``): the search that ends hypotheses at SEP -- a push returns rank 0
    [batch, max_len] and ``last_predictions`` [batch, n, max_len], ``last_scores`` / ``last_lengths`` [batch, n] hold all ranks."""

    def __init__(self, model, batch, hop, max_len, mode, beams, gate=None, carry=False, logprobs=False, top_logprobs=0, partial=False,
                 constraints=None, prompt=None, search=None):
        self._carry, self._prev, self._beams = bool(carry), None, beams
        self._se = search
        self.last_predictions = self.last_scores = self.last_lengths = None
        self._co = constraints
        self._batch = int(batch)
        self._pr = None
        self._m, self._max_len = model, max_len          # (the prompt setter needs them; the base class sets them again)
        self.prompt = prompt
        self._partial = bool(partial)
        self.last_frames = None          # frames per clip the caption of the last push saw (mem_tokens unless partial=True)
        self._stats = dict(captions=0, draft_tokens=0, accepted=0, tail_steps=0)
        super().__init__(model, WindowSchedule(batch, model.cfg.mem_tokens, hop, partial=self._partial), max_len, mode, gate, logprobs, top_logprobs)

    @property
    def prompt(self):
        """The stream's prompt as normalised ids int64 [batch, P] on the device (CLS first; rows padded with CLS), or None."""
        return None if self._pr is None else self._pr.ids

    @prompt.setter
    def prompt(self, value):
        if value is not None and self._carry:
            raise ValueError("carry=True is not combined with prompt= or the constraint arguments")
        limit = self._max_len if self._beams is None else self._max_len - 1
        self._pr = self._m._prompt(value, None, self._batch, limit, "max_len" if self._beams is None else "max_len - 1")

    @property
    def prompt_lengths(self):
        return None if self._pr is None else self._pr.lengths

    def _reset_lib(self):
        with torch.cuda.device(self._m._dev):
            self._m._call("gitcap_student_window_reset", self._sched.batch)

    def _clear(self):
        self._prev = None                                # the next caption is a plain call

    def stats(self) -> dict:
        """Since the stream was opened: ``captions`` returned, ``draft_tokens`` offered to the verify pass (per clip; 0 for a
        caption decoded by the plain call), ``accepted`` of them (the minimum over the clips, as the loop advances them in
        lockstep), ``tail_steps`` decoded one by one behind a draft (a plain call's steps are not counted), and ``last`` = the
        same three numbers of the latest caption.  A gate keeps its own statistics (FrameGate.stats)."""
        return dict(self._stats)

    def _tokens(self, frames: torch.Tensor) -> torch.Tensor:
        """One frame per clip ([B,H,W,3] uint8 / [B,3,S,S] fp32), n of them ([B,n,...]) or memory tokens [B,n,d_model]
        -> memory tokens [B,n,d_model] fp32 on the device."""
        m = self._m
        if frames.dtype != torch.uint8 and frames.dim() == 3:
            if frames.shape[2] != m.cfg.d_model:
                raise ValueError(f"expected memory tokens [B,n,{m.cfg.d_model}], got {tuple(frames.shape)}")
            return frames.to(device=m._dev, dtype=torch.float32).contiguous()
        if frames.dim() == 4:
            frames = frames.unsqueeze(1)
        if frames.dim() != 5:
            raise ValueError(f"expected frames [B,H,W,3] uint8, [B,3,S,S] fp32, [B,n,...] or tokens [B,n,d_model], got {tuple(frames.shape)}")
        self._sched.check(frames.shape[0], frames.shape[1])          # before any device work
        return m.image_encoder.memory(frames).contiguous()

    def _push(self, frames: torch.Tensor, to_cpu: bool):
        """frames: see ``_tokens``; only these frames are encoded.  -> None, or the caption of the window when one is due: greedy
        ids [B, 1+steps] (truncated as in greedy_decode), or with ``beams`` the best beam [B, max_len]."""
        m = self._m
        mem = self._tokens(frames)
        B, n = mem.shape[:2]
        self._sched.check(B, n)
        with torch.cuda.device(m._dev):
            m._call("gitcap_student_window_push", _lib.ptr(mem), B, n, m._stream())
        if not self._sched.push(B, n):
            return None
        with torch.cuda.device(m._dev):
            if self._beams is None:
                ids, steps, lp = self._greedy_buffers(B)
                tk = self._topk_buffers(B)
                last = dict(draft_tokens=0, accepted=0, tail_steps=0)
                if self._carry and self._prev is not None:
                    last = m._draft_call("gitcap_student_window_greedy_draft", (), self._prev, self._max_len, self._mode, ids, steps, lp)
                else:
                    m._attach_logprobs(lp, tk)
                    if self._co is not None:
                        self._co.attach(m)
                    if self._pr is not None:
                        self._pr.attach(m)
                    if self._partial:            # whatever the window holds; a full one is the plain call
                        seen = ctypes.c_int32(0)
                        m._call("gitcap_student_window_greedy_partial", self._max_len, self._mode, _lib.ptr(ids), _lib.ptr(steps),
                                ctypes.byref(seen), m._stream())
                        self.last_frames = int(seen.value)
                    else:
                        m._call("gitcap_student_window_greedy", self._max_len, self._mode, _lib.ptr(ids), _lib.ptr(steps), m._stream())
                out = self._finish_greedy(ids, steps, lp, to_cpu, tk)
                if self._carry:
                    self._prev = ids[:, :out.shape[1]]       # stays on the device, truncated as the caption is
                for k, v in last.items():
                    self._stats[k] += v
                self._stats["last"] = last
            else:
                if self._co is not None:
                    self._co.attach(m)
                if self._pr is not None:
                    self._pr.attach(m)
                call = lambda ptr: m._call("gitcap_student_window_beam_search", self._beams, self._max_len, ptr, m._stream())
                if self._se is not None:
                    res = self._se.run(m, B, self._max_len, call)
                    if to_cpu:
                        res = {name: t.cpu() for name, t in res.items()}
                    self.last_predictions, self.last_scores, self.last_lengths = res["predictions"], res["scores"], res["lengths"]
                    out = self.last_predictions[:, 0]
                else:
                    ids = torch.empty((B, self._max_len), dtype=torch.int64, device=m._dev)
                    call(_lib.ptr(ids))
                    out = ids.cpu() if to_cpu else ids
        if not self._partial:
            self.last_frames = m.cfg.mem_tokens
        self._stats["captions"] += 1
        return out


def _rebuild_student(cfg_dict, weights, kwargs, encoder=None):
    return StudentCaptioner(cfg=StudentConfig(**cfg_dict), weights=weights, image_encoder=encoder, **kwargs)


class StudentCaptioner(_NativeModule):
    _PREFIX, _FINALIZE = "gitcap_student", "gitcap_student_finalize"

    def __init__(self, image_enc_name: Optional[str] = None, d_model: int = 576, n_head: int = 8, d_ffn: int = 1024,
                 dropout: float = 0.0, num_decoder_layers: int = 2, vocab_length: int = 30522, cls_token_id: int = 101,
                 sep_token_id: int = 102, *, cfg: Optional[StudentConfig] = None,
                 weights: Optional[Mapping[str, np.ndarray]] = None, image_encoder=None,
                 device: str | torch.device = "cuda:0", max_batch: int = 16, max_text_len: int = 32,
                 mem_tokens: int = 6, stop: str = "all_sep"):
        super().__init__()
        if cfg is None:
            cfg = StudentConfig(d_model=d_model, n_head=n_head, d_ffn=d_ffn, num_decoder_layers=num_decoder_layers,
                                vocab_length=vocab_length, cls_token_id=cls_token_id, sep_token_id=sep_token_id,
                                mem_tokens=mem_tokens)
        cfg.validate()
        self.cfg = cfg
        self.image_enc_name = image_enc_name
        self._kw = dict(max_batch=int(max_batch), max_text_len=int(max_text_len), stop=stop)
        if isinstance(image_encoder, str):
            if image_encoder != "native":
                raise ValueError(f"image_encoder={image_encoder!r}: only 'native' (or a module) is accepted")
            image_encoder = TinyViTEncoder(tinyvit_config(image_enc_name or "tiny_vit_21m_224"), device=device,
                                           max_frames=int(max_batch) * cfg.mem_tokens)
        if isinstance(image_encoder, TinyViTEncoder) and image_encoder.out_dim != cfg.d_model:
            raise ValueError(f"the TinyViT encoder's last width {image_encoder.out_dim} != d_model {cfg.d_model}")
        self.image_encoder = image_encoder
        self.cls_token_id, self.sep_token_id = cfg.cls_token_id, cfg.sep_token_id
        self.n_head = cfg.n_head
        self.stop = stop
        self._dev = torch.device(device)
        self._handle = None
        self._window_owner = None                       # token of the live StudentCaptionStream
        self._pool_owner = None                         # token of the live StudentStreamPool (state of its own beside the window)
        self.last_accepted: Optional[int] = None        # draft tokens the last greedy_decode(draft=...) accepted
        self._weights: Optional[Dict[str, np.ndarray]] = None
        self._lib = _lib.load()                         # raises if libgitcap.so is missing
        self._open()
        if weights is not None:
            self.load_state_dict(weights)

    # ------------------------------------------------------------------ handle management
    def _cconfig(self):
        self.max_batch, self.max_text_len = self._kw["max_batch"], self._kw["max_text_len"]
        return CStudentConfig.from_config(self.cfg, self.max_batch, self.max_text_len)

    def _moved(self):
        self._window_owner = None                       # the window lived in the old handle
        self._pool_owner = None                         # and so did the pool

    # ------------------------------------------------------------------ nn.Module surface
    def to(self, *args, **kwargs):
        super().to(*args, **kwargs)
        if self._device_arg(args, kwargs) is not None and self.image_encoder is not None:
            self.image_encoder.to(self._dev)            # whether or not the decoder had to move
        return self

    def _native(self) -> bool:
        return isinstance(self.image_encoder, TinyViTEncoder)

    def state_dict(self, *a, **k):
        sd = super().state_dict()
        if self._native():
            sd.update({ENC_PREFIX + n: v for n, v in self.image_encoder.state_dict().items()})
        return sd

    def load_state_dict(self, state_dict, strict: bool = True):
        """Takes the reference's checkpoint keys as they are (src/inference.py:38).  Keys outside the decoder
        (image_encoder.*, projectors.*, upsample, project, project_decoder, the unused template
        ``decoder_layer.*``) are ignored; a missing ``pos_enc.pe`` buffer is rebuilt from model.py:324-335.
        With a native TinyViT encoder the ``image_encoder.model.*`` keys load into it: a missing encoder key is an
        error, unless the checkpoint has no encoder key at all and the encoder already holds weights."""
        if self._native():
            enc = {k[len(ENC_PREFIX):]: v for k, v in state_dict.items() if k.startswith(ENC_PREFIX)}
            if enc or not self.image_encoder.loaded:
                if not enc:
                    raise KeyError(f"missing TinyViT encoder weights ({ENC_PREFIX}*) for image_encoder='native'")
                self.image_encoder.load_state_dict(enc)
        w = {}
        for name, shape in student_shapes(self.cfg).items():
            if name not in state_dict:
                if name == "pos_enc.pe":
                    w[name] = positional_table(self.cfg.d_model, self.cfg.max_pos)
                    continue
                raise KeyError(f"missing student weight {name}")
            w[name] = self._as_f32(state_dict[name])
        check_student_shapes(self.cfg, w)
        self._upload(w)
        self._weights = w
        return self

    def _upload(self, w):
        self._pool_owner = None                         # gitcap_student_finalize releases the pool: its K|V rows came from the old weights
        self._load_tensors((name, w[name]) for name in student_shapes(self.cfg))

    def __reduce__(self):
        if self.image_encoder is not None and not self._native():
            raise TypeError("pickle the image encoder separately; StudentCaptioner pickles its decoder and a native encoder only")
        from dataclasses import asdict
        kw = dict(self._kw)
        kw["device"] = str(self._dev)
        kw["image_enc_name"] = self.image_enc_name
        return _rebuild_student, (asdict(self.cfg), self._weights, kw, self.image_encoder)

    # ------------------------------------------------------------------ clips of different length (gitcap/ragged.py)
    def _frame_limit(self) -> int:
        """The most frames a clip may have (what gitcap.sampling.caption_videos asks the sampler for)."""
        return self.cfg.mem_tokens

    @staticmethod
    def _is_ragged(src, frame_counts) -> bool:
        return frame_counts is not None or not isinstance(src, torch.Tensor)

    @staticmethod
    def _nclips(src) -> int:
        return src.shape[0] if isinstance(src, torch.Tensor) else len(src)

    def _encode_packed(self, frames: torch.Tensor) -> torch.Tensor:
        """Packed frames [n,3,S,S] (or uint8 [n,H,W,3]) -> memory tokens [n, D] from one encode: no frame is padded."""
        if self._native():
            enc = self.image_encoder
            return enc._encode(enc._frames(frames), False)[1]
        if frames.dtype == torch.uint8:
            raise _lib.GitcapError("uint8 camera frames need the native TinyViT encoder (image_encoder='native'): the frame "
                                   "transform runs inside its first convolution")
        if self.image_encoder is None:
            raise _lib.GitcapError("StudentCaptioner was built without an image_encoder: pass image_encoder='native' (the "
                                   "TinyViT encoder of libgitcap) or a module, or call the decoder with memory [F_b, d_model] per clip")
        return torch.mean(self.image_encoder(frames.to(self._dev))[-1], dim=[2, 3])

    def _clip_memories(self, src, frame_counts):
        """The ragged input forms -> (memory tokens [F_b, D] fp32 on the device, one tensor per clip; the counts; src's device).
        ``src``: a list of B clips -- frames [F_b,3,S,S], uint8 camera frames [F_b,H,W,3] or memory [F_b,D] -- or a padded tensor
        [B,Fmax,...] of one of the three with ``frame_counts`` [B] (what lies beyond a clip's count is ignored).  1 <= F_b <=
        mem_tokens.  Frames are encoded packed, sum(counts) of them in one pass."""
        F, D = self.cfg.mem_tokens, self.cfg.d_model
        padded = isinstance(src, torch.Tensor)
        is_mem = (src.dim() == 3 if padded else bool(len(src)) and all(isinstance(p, torch.Tensor) and p.dim() == 2 for p in src))
        if is_mem and (src.dtype if padded else src[0].dtype) != torch.uint8:
            if padded:
                if frame_counts is None:
                    raise ValueError("a padded tensor needs frame_counts")
                counts = ragged.check_counts(frame_counts, src.shape[0], min(F, src.shape[1]))
                parts = [src[b, :n] for b, n in enumerate(counts)]
            else:
                parts = list(src)
                counts = ragged.check_counts([p.shape[0] for p in parts], len(parts), F)
                if frame_counts is not None and ragged.check_counts(frame_counts, len(parts), F) != counts:
                    raise ValueError("frame_counts disagrees with the clips' own frame counts")
            if any(p.shape[-1] != D or p.dtype == torch.uint8 for p in parts):
                raise ValueError(f"expected memory tokens [F_b, {D}] per clip")
            out_dev = parts[0].device
            mems = [p.to(device=self._dev, dtype=torch.float32) for p in parts]
        else:
            size = self.image_encoder.cfg.img_size if self._native() else (src.shape[-1] if padded else src[0].shape[-1])
            parts, counts, _ = ragged.clips(src, frame_counts, size, F)
            out_dev = parts[0].device
            mems = list(self._encode_packed(ragged.pack(parts)).split(counts, 0))
        if len(counts) > self.max_batch:
            raise ValueError(f"batch {len(counts)} outside 1..max_batch={self.max_batch}")
        return mems, counts, out_dev

    def _ragged_memory(self, src, frame_counts, n: int = 1):
        """-> (memory for the library, rows, counts or None, src's device): n rows per clip (candidates: rows whose memory is
        repeated).  Every clip of mem_tokens frames: the dense [rows, F, D] of the existing calls, counts None.  Else the packed
        [sum, D] rows and the per-row counts gitcap_student_attach_frame_counts takes."""
        mems, counts, out_dev = self._clip_memories(src, frame_counts)
        if n > 1:
            mems = [m for m in mems for _ in range(n)]
            counts = [c for c in counts for _ in range(n)]
        if all(c == self.cfg.mem_tokens for c in counts):
            return torch.stack(mems, 0).contiguous(), len(counts), None, out_dev
        return torch.cat(mems, 0).contiguous(), len(counts), counts, out_dev

    def _attach_counts(self, counts):
        """One-shot: the next call that takes memory reads it packed (gitcap_student_attach_frame_counts; the counts are copied)."""
        if counts is not None:
            self._call("gitcap_student_attach_frame_counts", (ctypes.c_int32 * len(counts))(*counts), len(counts))

    def _set_memory(self, src, frame_counts=None, n: int = 1) -> int:
        """``src`` (any input form, n rows per clip) becomes the handle's memory -> its rows."""
        if self._is_ragged(src, frame_counts):
            mem, rows, counts, _ = self._ragged_memory(src, frame_counts, n)
        else:
            mem, counts = self._memory(self._src_memory(src)), None
            mem = mem.repeat_interleave(n, dim=0) if n > 1 else mem
            rows = mem.shape[0]
        self._attach_counts(counts)
        self._call("gitcap_student_set_memory", _lib.ptr(mem), rows, self._stream())
        return rows

    @staticmethod
    def _clip_range(src, frame_counts, b0, b1):
        """Clips b0 .. b1 - 1 of either input form."""
        return src[b0:b1], None if frame_counts is None else frame_counts[b0:b1]

    # ------------------------------------------------------------------ reference API
    def _memory(self, memory: torch.Tensor) -> torch.Tensor:
        if memory.dim() != 3 or memory.shape[1] != self.cfg.mem_tokens or memory.shape[2] != self.cfg.d_model:
            raise ValueError(f"expected memory [B,{self.cfg.mem_tokens},{self.cfg.d_model}], got {tuple(memory.shape)}")
        if memory.shape[0] == 0 or memory.shape[0] > self.max_batch:
            raise ValueError(f"batch {memory.shape[0]} outside 1..max_batch={self.max_batch}")
        return memory.to(device=self._dev, dtype=torch.float32).contiguous()

    def _frames_memory(self, src: torch.Tensor) -> torch.Tensor:
        """frames [B,F,C,H,W] (or uint8 camera frames [B,F,H,W,3]) -> memory [B,F,D]; the native encoder writes no feature
        maps and does not sync."""
        if self._native():
            return self.image_encoder.memory(src)
        return self.forward_image_enc(src)[1]

    def _src_memory(self, src: torch.Tensor) -> torch.Tensor:
        """The ``src`` of the decode calls: frames (5-D, or uint8 of either rank) go through the encoder, else memory."""
        return self._frames_memory(src) if src.dim() == 5 or src.dtype == torch.uint8 else src

    @torch.no_grad()
    def forward_image_enc(self, x: torch.Tensor, frame_counts=None):
        """model.py:108-126: frames [B,F,C,H,W] -> (feature maps, memory [B,F,De]) through the image encoder.  The native
        encoder also takes uint8 BGR camera frames [B,F,H,W,3].
        frame_counts (or ``x`` as a list of B clips [F_b, ...]): clips that differ in length, encoded packed -> (feature maps
        [sum(counts),Ci,Hi,Wi], memory [B,Fmax,De] with zeros beyond a clip's frames, valid bool [B,Fmax])."""
        if self._is_ragged(x, frame_counts):
            size = self.image_encoder.cfg.img_size if self._native() else (x.shape[-1] if isinstance(x, torch.Tensor) else x[0].shape[-1])
            parts, counts, _ = ragged.clips(x, frame_counts, size, self.cfg.mem_tokens)
            packed = ragged.pack(parts)
            if self._native():
                enc = self.image_encoder
                fmaps, mem = enc._encode(enc._frames(packed), True)
            else:
                if self.image_encoder is None or packed.dtype == torch.uint8:
                    raise _lib.GitcapError("frames need an image_encoder (uint8 camera frames the native one)")
                fmaps = self.image_encoder(packed.to(self._dev))
                mem = torch.mean(fmaps[-1], dim=[2, 3])
            memory, valid = ragged.unpack_rows(mem, counts, 1)
            return fmaps, memory, valid
        if self._native():
            return self.image_encoder.forward_with_memory(x)
        if x.dtype == torch.uint8:
            raise _lib.GitcapError("uint8 camera frames need the native TinyViT encoder (image_encoder='native'): the frame "
                                   "transform runs inside its first convolution")
        if self.image_encoder is None:
            raise _lib.GitcapError("StudentCaptioner was built without an image_encoder: pass image_encoder='native' (the "
                                   "TinyViT encoder of libgitcap) or a module, or call the decoder with memory [B,F,d_model]")
        s = x.shape
        fmaps = self.image_encoder(x.to(self._dev).view(s[0] * s[1], *s[2:]))
        memory = torch.mean(fmaps[-1], dim=[2, 3]).view(s[0], s[1], -1)
        return fmaps, memory

    @torch.no_grad()
    def forward_decoder(self, y: torch.Tensor, memory: torch.Tensor, frame_counts=None) -> torch.Tensor:
        """model.py:128-154: y [B,T] ids, memory [B,F,D] -> logits [B,T,V] (fp32, on the device).
        frame_counts (memory padded [B,Fmax,D]), or memory as a list of B tensors [F_b,D]: clips that differ in length; row b
        attends to its own F_b tokens only."""
        counts = None
        if self._is_ragged(memory, frame_counts):
            mem, _, counts, _ = self._ragged_memory(memory, frame_counts)
        else:
            mem = self._memory(memory)
        ids = y.to(device=self._dev, dtype=torch.int64).contiguous()
        B, T = ids.shape
        if B != (mem.shape[0] if counts is None else len(counts)):
            raise ValueError("y and memory disagree on the batch size")
        if T < 1 or T > self.max_text_len + 1:
            raise ValueError(f"T={T} outside 1..max_text_len+1={self.max_text_len + 1}")
        logits = torch.empty((B, T, self.cfg.vocab_length), dtype=torch.float32, device=self._dev)
        with torch.cuda.device(self._dev):
            self._attach_counts(counts)
            self._call("gitcap_student_set_memory", _lib.ptr(mem), B, self._stream())
            self._call("gitcap_student_forward_decoder", _lib.ptr(ids), T, B, T, _lib.ptr(logits), self._stream())
        return logits

    @torch.no_grad()
    def score(self, x: torch.Tensor, y: torch.Tensor, *, lengths: Optional[torch.Tensor] = None, until_sep: bool = True,
              ignore_id: Optional[int] = None, return_top1: bool = False, top_k: int = 0, frame_counts=None) -> dict:
        """GitCaptioner.score over the student decoder (include/gitcap.h: gitcap_student_score): ``x`` frames or memory [B,F,D],
        ``y`` CLS-first ids [B, T] or [B, n, T] (n candidates per clip: rows whose memory is repeated).  Same ignore rules and
        the same dict (``top_k`` included); clips go through in chunks of max_batch // n.
        frame_counts (or ``x`` as a list of clips; as in greedy_decode): clips that differ in length."""
        from . import scoring
        top_k = scoring.check_top_k(top_k)
        ids, had_n = scoring.candidates(y, self._dev)
        B, n, T = ids.shape
        if self._nclips(x) != B:
            raise ValueError("x and y disagree on the number of clips")
        if T > self.max_text_len + 1:
            raise ValueError(f"T={T} > max_text_len+1={self.max_text_len + 1}")
        if n > self.max_batch:
            raise ValueError(f"{n} candidates per clip > max_batch={self.max_batch} rows the handle was created for")
        ln = scoring.row_lengths(ids, self.cfg.sep_token_id, until_sep, lengths)
        Bc = min(B, self.max_batch // n)
        chunks = []
        with torch.cuda.device(self._dev):
            for b0 in range(0, B, Bc):
                b1 = min(B, b0 + Bc)
                rows = self._set_memory(*self._clip_range(x, frame_counts, b0, b1), n)
                buf = scoring.ScoreBuffers(rows, T, self._dev, return_top1, top_k)
                cid = ids[b0:b1].reshape(rows, T)
                cl = None if ln is None else ln[b0:b1].reshape(rows).contiguous()
                buf.attach_topk(self._call, "gitcap_student_attach_top_logprobs")
                self._call("gitcap_student_score", _lib.ptr(cid), T, rows, T, _lib.ptr(cl), -1 if ignore_id is None else int(ignore_id),
                           *buf.args(T), self._stream())
                chunks.append(buf)
        return scoring.result(chunks, B, n, had_n, return_top1, x.device if isinstance(x, torch.Tensor) else x[0].device)

    @torch.no_grad()
    def attention(self, x: torch.Tensor, y: torch.Tensor, *, layer: Optional[int] = None, lengths: Optional[torch.Tensor] = None,
                  until_sep: bool = True, frame_counts=None) -> dict:
        """Which frame every token of GIVEN captions comes from (include/gitcap.h: gitcap_student_attention).  The student's memory
        is one token per frame, so its cross-attention is the attribution: ``frame_attention`` fp32 [B, (n,) T-1, F], the
        cross-attention probabilities averaged over the heads and over all layers (``layer=None``) or one; each position's F
        values sum to 1.  ``x``, ``y``, ``lengths``, ``until_sep`` as in score; index j is the position that predicts
        y[..., j + 1]; positions behind a row's length hold zeros.  One teacher-forced pass (score's, without the head).
        frame_counts (or ``x`` as a list of clips; as in greedy_decode): clips that differ in length; F stays mem_tokens and the
        columns from a clip's count on hold 0."""
        from . import scoring
        ids, had_n = scoring.candidates(y, self._dev)
        B, n, T = ids.shape
        if self._nclips(x) != B:
            raise ValueError("x and y disagree on the number of clips")
        if T < 2 or T > self.max_text_len + 1:
            raise ValueError(f"T={T} outside 2..max_text_len+1={self.max_text_len + 1}")
        if n > self.max_batch:
            raise ValueError(f"{n} candidates per clip > max_batch={self.max_batch} rows the handle was created for")
        lay = -1 if layer is None else int(layer)
        if not -1 <= lay < self.cfg.num_decoder_layers:
            raise ValueError(f"layer={layer} outside 0..{self.cfg.num_decoder_layers - 1}")
        ln = scoring.row_lengths(ids, self.cfg.sep_token_id, until_sep, lengths)
        Bc = min(B, self.max_batch // n)
        F = self.cfg.mem_tokens
        outs = []
        with torch.cuda.device(self._dev):
            for b0 in range(0, B, Bc):
                b1 = min(B, b0 + Bc)
                rows = self._set_memory(*self._clip_range(x, frame_counts, b0, b1), n)
                cid = ids[b0:b1].reshape(rows, T)
                cl = None if ln is None else (ln[b0:b1].reshape(rows) - 1).clamp_(min=0).to(torch.int32).contiguous()
                fm = torch.empty((rows, T - 1, F), dtype=torch.float32, device=self._dev)
                self._call("gitcap_student_attention", _lib.ptr(cid), T, rows, T - 1, lay, _lib.ptr(cl), _lib.ptr(fm), F, self._stream())
                outs.append(fm)
        shape = (B, n) if had_n else (B,)
        return dict(frame_attention=torch.cat(outs, 0).reshape(*shape, T - 1, F).to(x.device if isinstance(x, torch.Tensor) else x[0].device))

    def forward(self, x: torch.Tensor, y: torch.Tensor):
        """model.py:99-106: feature maps + [logits]."""
        fmaps, memory = self.forward_image_enc(x)
        return list(fmaps) + [self.forward_decoder(y, memory)]

    def _attach_logprobs(self, lp: Optional[torch.Tensor], tk=None):
        """One-shot: the next greedy-family call writes its per-token log-probabilities to ``lp`` (fp32 [B, max_len], contiguous)
        and the k best alternatives per step to ``tk`` = (int64, fp32) [B, max_len, k] (a draft call refuses these)."""
        if lp is not None:
            self._call("gitcap_student_attach_token_logprobs", _lib.ptr(lp), lp.shape[1])
        if tk is not None:
            self._call("gitcap_student_attach_top_logprobs", tk[0].shape[2], _lib.ptr(tk[0]), _lib.ptr(tk[1]), tk[0].shape[1])

    def _constraints(self, no_repeat_ngram_size, min_length, suppress_tokens, max_len, need=1):
        """The constraint arguments of the decoding calls -> _StudentConstraints or None (the defaults: nothing is attached).
        ValueError for what the library would refuse (include/gitcap.h: gitcap_student_attach_constraints), before anything is
        launched.  need: the columns a row must keep (1: the arg-max; k: a clip's beam candidates)."""
        from .search import check_constraints
        n, m, sup = check_constraints(no_repeat_ngram_size, min_length, suppress_tokens)
        if not (n or m or sup):
            return None
        if len(sup) + max_len + need > self.cfg.vocab_length:
            raise ValueError(f"{len(sup)} suppressed ids over {max_len} steps could ban every column of a row (vocab_size {self.cfg.vocab_length})")
        if self.cfg.vocab_length > 131072:
            raise ValueError("the constraints' ban mask takes a vocabulary of at most 131072 columns")
        return _StudentConstraints(self, n, m, sup)

    def _draft_call(self, name, head, draft: torch.Tensor, max_len: int, mode: int, ids: torch.Tensor, steps: torch.Tensor,
                    lp: Optional[torch.Tensor] = None, tk=None) -> dict:
        """One of the two draft entry points (``head`` = the arguments in front of the draft's); ``draft`` int64 [B, 1+n] on
        either device, trimmed to max_len columns beyond CLS.  -> what the call offered, accepted and decoded behind it.
        ``lp``: see _attach_logprobs."""
        B = ids.shape[0]
        if draft.dim() != 2 or draft.shape[0] != B or draft.shape[1] < 2 or draft.dtype != torch.int64:
            raise ValueError(f"draft must be int64 [{B}, 1+n] with n >= 1, got {draft.dtype} {tuple(draft.shape)}")
        d = draft[:, :1 + max_len].to(self._dev).contiguous()
        n = d.shape[1] - 1
        acc = ctypes.c_int32(-1)
        before = self._draft_stats()
        self._attach_logprobs(lp, tk)
        self._call(name, *head, _lib.ptr(d), n + 1, n, max_len, mode, _lib.ptr(ids), _lib.ptr(steps), ctypes.byref(acc), self._stream())
        self.last_accepted = int(acc.value)
        return dict(draft_tokens=n, accepted=self.last_accepted, tail_steps=self._draft_stats()[3] - before[3])

    def _draft_stats(self):
        """gitcap_student_draft_stats: (draft calls, tokens offered, tokens accepted, tail steps) of this handle."""
        out = (ctypes.c_int64 * 4)()
        self._call("gitcap_student_draft_stats", out)
        return tuple(int(v) for v in out)

    @torch.no_grad()
    def greedy_decode(self, src: torch.Tensor, max_len: int = 10, stop: Optional[str] = None,
                      draft: Optional[torch.Tensor] = None, return_logprobs: bool = False, top_logprobs: int = 0,
                      return_attention: bool = False, frame_counts=None, no_repeat_ngram_size: int = 0, min_length: int = 0,
                      suppress_tokens=None, prompt=None, prompt_lengths=None):
        """model.py:156-187.  ``src``: frames [B,F,C,H,W] (needs ``image_encoder``; a native one keeps the memory on the
        device and also takes uint8 camera frames [B,F,H,W,3]) or memory [B,F,D].
        Returns int64 [B, 1+steps] starting with CLS, on ``src``'s device.
        ``draft``: int64 [B, 1+n], a guess at the result (e.g. the previous caption of a live stream; column 0 is taken as CLS,
        any ids are allowed).  The result is the one without it, bit for bit: the draft is verified in one pass, the tokens the
        loop would have produced anyway are accepted (``last_accepted`` = their number) and only the rest is decoded step by
        step (include/gitcap.h: gitcap_student_greedy_draft).  The call waits on the host for the verify pass.
        ``return_logprobs``: -> (ids, logprobs), logprobs fp32 [B, steps] on ``src``'s device, column t =
        log_softmax(step t's logits)[ids[:, t + 1]]; with a ``draft`` bit for bit the values without it.
        ``top_logprobs=k`` (1..32): the result gains ``top_ids`` int64 / ``top_logprobs`` fp32 [B, steps, k] behind ids (and
        logprobs): every step's k best tokens by (logit descending, id ascending) and their log-probabilities; rank 0 is the
        emitted token.  No logits tensor is written (include/gitcap.h: gitcap_attach_top_logprobs).  A ``draft`` call refuses it.
        ``return_attention``: the result gains, last, ``frame_attention`` fp32 [B, steps, F] (see attention()), from one
        teacher-forced pass over the result behind the loop: bit for bit attention(src, ids, until_sep=False).
        frame_counts: clips that differ in length -- ``src`` padded [B,Fmax,...] (frames, camera frames or memory) with
        frame_counts [B], or ``src`` as a list of B clips [F_b,3,S,S] / uint8 [F_b,H,W,3] / memory [F_b,D], 1 <= F_b <=
        mem_tokens.  The batch runs packed, without padding or masking (include/gitcap.h: gitcap_student_attach_frame_counts):
        every clip's results are bit for bit those of the clip decoded alone by a model with mem_tokens = F_b.
        no_repeat_ngram_size / min_length / suppress_tokens: hard constraints on what a step may emit (include/gitcap.h:
        gitcap_student_attach_constraints; HF's NoRepeatNGram / MinLength / SuppressTokens processors): no n-gram of the row so far
        (CLS included) twice, no SEP while the row is shorter than min_length (CLS counts), and up to 256 ids never.  Banned columns
        are -inf before the arg-max, so ``return_logprobs`` / ``top_logprobs`` are those of the renormalised row and never name a
        banned id.  The loop keeps decoding behind a row's SEP and the rules keep applying there.  Not combined with ``draft``.
        prompt / prompt_lengths: a text prefix per clip (include/gitcap.h: gitcap_student_attach_prompt; GitCaptioner.greedy_decode's
        argument): int64 [B, P], optionally with prompt_lengths [B], or a list of B 1-D tensors of different lengths; CLS is
        prepended where missing, and a row of CLS alone has no prompt.  The result includes the prompt: row b starts with its
        lengths[b] prompt tokens and the model's tokens follow; log-probabilities are 0.0 at a prompt's positions, ``top_logprobs``
        reports the model's own ranks there, a prompt token is emitted even when a constraint bans it and does not count for the
        stop rule.  At most max_len tokens (CLS included).  Not combined with ``draft``."""
        if not 0 <= int(top_logprobs) <= 32:
            raise ValueError(f"top_logprobs={top_logprobs} outside 0..32")
        if draft is not None and (prompt is not None or _constrained(no_repeat_ngram_size, min_length, suppress_tokens)):
            raise ValueError("draft= is not combined with prompt= or the constraint arguments")
        counts = None
        if self._is_ragged(src, frame_counts):
            mem, B, counts, out_dev = self._ragged_memory(src, frame_counts)
        else:
            out_dev = src.device
            memory = self._src_memory(src)
            mem = self._memory(memory)
            B = mem.shape[0]
        if max_len < 1 or max_len > self.max_text_len:
            raise ValueError(f"max_len={max_len} outside 1..max_text_len={self.max_text_len}")
        mode = {"all_sep": STOP_ALL_SEP, "never": STOP_NEVER}[stop or self.stop]
        co = self._constraints(no_repeat_ngram_size, min_length, suppress_tokens, max_len)
        pr = self._prompt(prompt, prompt_lengths, B, max_len, "max_len")
        ids = torch.empty((B, max_len + 1), dtype=torch.int64, device=self._dev)
        steps = torch.zeros(1, dtype=torch.int32, device=self._dev)
        lp = torch.empty((B, max_len), dtype=torch.float32, device=self._dev) if return_logprobs else None
        tk = None
        if top_logprobs:
            tk = (torch.empty((B, max_len, int(top_logprobs)), dtype=torch.int64, device=self._dev),
                  torch.empty((B, max_len, int(top_logprobs)), dtype=torch.float32, device=self._dev))
        with torch.cuda.device(self._dev):
            self._attach_counts(counts)
            if draft is not None:
                self._draft_call("gitcap_student_greedy_draft", (_lib.ptr(mem), B), draft, max_len, mode, ids, steps, lp, tk)
            else:
                self._attach_logprobs(lp, tk)
                if co is not None:
                    co.attach(self)
                if pr is not None:
                    pr.attach(self)
                self._call("gitcap_student_greedy", _lib.ptr(mem), B, max_len, mode, _lib.ptr(ids), _lib.ptr(steps), self._stream())
        n = int(steps.item()) if mode == STOP_ALL_SEP else max_len
        ids = ids[:, :1 + n]
        mv = lambda t: t.to(out_dev) if out_dev != t.device else t
        out = (mv(ids),)
        if lp is not None:
            out += (mv(lp[:, :n]),)
        if tk is not None:
            out += (mv(tk[0][:, :n]), mv(tk[1][:, :n]))
        if return_attention:
            fm = torch.empty((B, n, self.cfg.mem_tokens), dtype=torch.float32, device=self._dev)
            if n:
                with torch.cuda.device(self._dev):      # the memory of the loop is still the handle's
                    self._call("gitcap_student_attention", _lib.ptr(ids), max_len + 1, B, n, -1, None, _lib.ptr(fm), self.cfg.mem_tokens,
                               self._stream())
            out += (mv(fm),)
        return out if len(out) > 1 else out[0]

    generate = greedy_decode

    @torch.no_grad()
    def beam_search(self, src: torch.Tensor, max_len: int = 10, k: int = 3, return_attention: bool = False, frame_counts=None,
                    no_repeat_ngram_size: int = 0, min_length: int = 0, suppress_tokens=None, prompt=None,
                    prompt_lengths=None, eos: bool = False, length_penalty: float = 1.0, num_keep_best: int = 1,
                    per_node_beam_size: Optional[int] = None, repetition_penalty: float = 1.0):
        """model.py:189-318: k beams without end-of-sequence handling; returns the best beam [B, max_len].
        ``eos=True``: the search that ends hypotheses at SEP instead (include/gitcap.h: gitcap_student_attach_search; the teacher's
        search rules): each step ranks k * per_node_beam_size candidates (default k per beam; 2..k, at most 16 in all, so k >= 2), a
        SEP candidate finishes its hypothesis with score = sum of log-probabilities / length ** length_penalty, a clip keeps its
        num_keep_best (1..k) best and stops extending once no live beam can beat them; ``repetition_penalty`` rewrites the logits
        of the tokens a row already holds.  Returns a dict: ``predictions`` int64 [B, n, max_len] (rank 0 best, SEP behind every
        hypothesis), ``scores`` fp32 [B, n] (-1e5 for a rank without a hypothesis) and ``lengths`` int32 [B, n] (tokens, CLS
        included, SEP not).  Combines with frame_counts, the constraint arguments and prompts.  Without ``eos=True`` the four
        search arguments must keep their defaults, and the call is today's, launch for launch.
        Runs on the device with the exact KV cache and no host round trip (``gitcap_student_beam_search``): the k beams
        of a clip are rows b*k+i (B*k <= max_batch), candidates are ranked by the beam top-k kernel, the cached K/V rows
        follow their beams.  frame_counts (or ``src`` as a list of clips; as in greedy_decode): clips that differ in length; the k
        beams of a clip share its memory rows.
        no_repeat_ngram_size / min_length / suppress_tokens (as in greedy_decode): every beam row's banned columns are -inf ahead of
        the log-softmax, so the scores renormalise over the allowed columns.
        prompt / prompt_lengths (as in greedy_decode; at most max_len - 1 tokens, CLS included): every beam of clip b starts from its
        prompt -- the search ranks nothing while the clip is inside it and the scores start behind it as they start behind CLS --
        and max_len counts the prompt; the result includes it."""
        if return_attention:
            raise ValueError("return_attention= is not taken by the beam family (beam_search) (its cache rows are not a caption's positions in order, or not the caller's to read yet): use attention(x, predictions) on the result")
        counts = None
        if self._is_ragged(src, frame_counts):
            mem, B, counts, out_dev = self._ragged_memory(src, frame_counts)
        else:
            out_dev = src.device
            memory = self._src_memory(src)
            mem = self._memory(memory)
            B = mem.shape[0]
        if B * k > self.max_batch:
            raise ValueError(f"B*k={B * k} rows > max_batch={self.max_batch}")
        if max_len - 1 > self.max_text_len:
            raise ValueError(f"max_len={max_len} exceeds max_text_len+1={self.max_text_len + 1}")
        if max_len < 2 or k < 1 or k > 16:
            raise ValueError("beam_search needs max_len >= 2 and 1 <= k <= 16")
        se = _search_options(eos, k, length_penalty, num_keep_best, per_node_beam_size, repetition_penalty)
        co = self._constraints(no_repeat_ngram_size, min_length, suppress_tokens, max_len, k if se is None else k * se.pn)
        pr = self._prompt(prompt, prompt_lengths, B, max_len - 1, "max_len - 1")
        call = lambda out: self._call("gitcap_student_beam_search", _lib.ptr(mem), B, k, max_len, out, self._stream())
        with torch.cuda.device(self._dev):
            self._attach_counts(counts)
            if co is not None:
                co.attach(self)
            if pr is not None:
                pr.attach(self)
            if se is not None:
                res = se.run(self, B, max_len, call)
                return {name: t.to(out_dev) if out_dev != t.device else t for name, t in res.items()}
            best = torch.empty((B, max_len), dtype=torch.int64, device=self._dev)
            call(_lib.ptr(best))
        return best.to(out_dev) if out_dev != best.device else best

    def caption_stream(self, batch: int = 1, hop: int = 1, max_len: int = 25, stop: Optional[str] = None,
                       beams: Optional[int] = None, gate: Optional[FrameGate] = None, carry: bool = False,
                       logprobs: bool = False, top_logprobs: int = 0, return_attention: bool = False,
                       partial: bool = False, no_repeat_ngram_size: int = 0, min_length: int = 0,
                       suppress_tokens=None, prompt=None, eos: bool = False, length_penalty: float = 1.0, num_keep_best: int = 1,
                       per_node_beam_size: Optional[int] = None, repetition_penalty: float = 1.0) -> StudentCaptionStream:
        """A sliding caption window over live frames (the reference's webcam loop): ``push(frames)`` appends
        frames of `batch` clips and returns the caption of the last ``mem_tokens`` frames once the window is full and `hop`
        frames have arrived since the last one, else None.  hop = mem_tokens is the reference's tumbling loop
        (real_time_inference.py:44-57), hop = 1 a caption per new frame.  Greedy by default (ids as
        greedy_decode(max_len, stop)); with ``beams`` the best beam of beam_search(max_len, k=beams).  Needs the native
        encoder.  One live stream per model: opening another one, or moving the model, invalidates this one.
        ``gate``: a FrameGate that decides on the device which pushed camera frames are worth encoding (it is reset here);
        without one every pushed frame is.
        ``carry``: a greedy stream passes its previous caption as the draft of the next window call (greedy_decode's ``draft``):
        the same captions; ``stats()`` tells how much of the drafts was accepted.  Not with ``beams``.
        ``logprobs`` (greedy streams only): after a push that returned a caption, ``stream.last_logprobs`` holds its per-token
        log-probabilities [B, steps] (greedy_decode's return_logprobs); works with ``gate`` and ``carry``.
        ``top_logprobs=k`` (greedy streams without ``carry``: a draft call does not carry alternatives): ``stream.last_top_ids`` /
        ``stream.last_top_logprobs`` [B, steps, k] of that caption (greedy_decode's top_logprobs).
        ``partial``: a caption is due once ``hop`` frames have arrived, whether or not the window is full: the first captions
        after a reset see the 1, 2, ... frames admitted so far (bit for bit greedy_decode on a list holding those frames), and
        from mem_tokens frames on the stream is the ``partial=False`` one.  ``stream.last_frames`` = the frames the last
        caption saw.  Works with ``gate``, ``logprobs`` and ``top_logprobs``; not with ``carry`` or ``beams``, whose window calls
        need a full window (include/gitcap.h: gitcap_student_window_greedy_partial).
        no_repeat_ngram_size / min_length / suppress_tokens (as in greedy_decode / beam_search): the stream's constraints, attached
        again for every caption, greedy or ``beams``; not with ``carry`` (a draft call does not take them).
        ``prompt`` (as in greedy_decode: [batch, P] or a list of `batch` 1-D tensors): one text prefix per stream row, kept for the
        stream's life and attached again for every caption, greedy or ``beams``; ``stream.prompt = ...`` replaces it,
        ``stream.prompt_lengths`` tells what of a caption row is prompt.  Not with ``carry``.
        ``eos`` / length_penalty / num_keep_best / per_node_beam_size / repetition_penalty (streams with ``beams``; as in
        beam_search): with ``eos=True`` a push returns the best hypothesis of every clip [batch, max_len], and
        ``stream.last_predictions`` [batch, n, max_len], ``stream.last_scores`` / ``stream.last_lengths`` [batch, n] hold all ranks:
        bit for bit beam_search(eos=True) on the window's frames."""
        if beams is None and (eos or length_penalty != 1.0 or num_keep_best != 1 or per_node_beam_size is not None or repetition_penalty != 1.0):
            raise ValueError("eos= and the search arguments are for streams with beams")
        if return_attention:
            raise ValueError("return_attention= is not taken by the window streams (caption_stream) (its cache rows are not a caption's positions in order, or not the caller's to read yet): use attention(x, predictions) on the result")
        if not 0 <= int(top_logprobs) <= 32:
            raise ValueError(f"top_logprobs={top_logprobs} outside 0..32")
        if top_logprobs and (beams is not None or carry):
            raise ValueError("top_logprobs is for greedy streams without carry")
        if logprobs and beams is not None:
            raise ValueError("logprobs=True is for greedy streams: it cannot be combined with beams")
        if carry and beams is not None:
            raise ValueError("carry=True verifies the previous greedy caption: it cannot be combined with beams")
        if carry and (prompt is not None or _constrained(no_repeat_ngram_size, min_length, suppress_tokens)):
            raise ValueError("carry=True is not combined with prompt= or the constraint arguments")
        if partial and (carry or beams is not None):
            raise ValueError("partial=True is for greedy streams without carry: the beam and draft window calls need a full window")
        if not self._native():
            raise _lib.GitcapError("caption_stream needs the native TinyViT encoder (image_encoder='native'): frames are "
                                   "encoded one at a time on the device")
        if batch < 1 or batch > self.max_batch:
            raise ValueError(f"batch {batch} outside 1..max_batch={self.max_batch}")
        mode = {"all_sep": STOP_ALL_SEP, "never": STOP_NEVER}[stop or self.stop]
        if beams is None:
            if max_len < 1 or max_len > self.max_text_len:
                raise ValueError(f"max_len={max_len} outside 1..max_text_len={self.max_text_len}")
        else:
            if batch * beams > self.max_batch:
                raise ValueError(f"batch*beams={batch * beams} rows > max_batch={self.max_batch}")
            if max_len < 2 or max_len - 1 > self.max_text_len or beams < 1 or beams > 16:
                raise ValueError(f"beam search needs 2 <= max_len <= max_text_len+1={self.max_text_len + 1} and 1 <= beams <= 16")
        if gate is not None:
            if not isinstance(gate, FrameGate):
                raise ValueError(f"gate must be a gitcap.framegate.FrameGate, got {type(gate).__name__}")
            gate.reset()
        se = None if beams is None else _search_options(eos, beams, length_penalty, num_keep_best, per_node_beam_size, repetition_penalty)
        co = self._constraints(no_repeat_ngram_size, min_length, suppress_tokens, max_len,
                               1 if beams is None else beams if se is None else beams * se.pn)
        return StudentCaptionStream(self, batch, hop, max_len, mode, beams, gate, carry, logprobs, top_logprobs, partial, co, prompt, se)

    def stream_pool(self, streams: int, hop: int = 1, max_len: int = 25, stop: Optional[str] = None, logprobs: bool = False,
                    top_logprobs: int = 0, min_frames: int = 1, no_repeat_ngram_size: int = 0, min_length: int = 0,
                    suppress_tokens=None, beams: Optional[int] = None, eos: bool = False, length_penalty: float = 1.0,
                    num_keep_best: int = 1, per_node_beam_size: Optional[int] = None,
                    repetition_penalty: float = 1.0) -> StudentStreamPool:
        """Several live cameras on one model (the multi-camera loop): `streams` independent windows of
        ``mem_tokens`` frames.  ``pool.push(frames, streams)`` takes n frames for any streams in any mix (frame i belongs to stream
        streams[i]), encodes them once in one packed pass and returns ``{stream: ids}`` for every stream that is due: at least
        `hop` of its frames have arrived since its last caption and it holds at least `min_frames` frames (1: a caption from a
        camera's first frame on, as caption_stream(partial=True); mem_tokens: only full windows, as partial=False).  The due
        streams are captioned as one ragged batch, in chunks of max_batch (include/gitcap.h: gitcap_student_pool_*).  A stream's
        caption is bit for bit greedy_decode(max_len, stop) on a list holding that stream's last frames, cut behind the row's own
        first SEP under the all_sep rule (not at the batch-wide step count): it does not depend on which other streams were due.
        ``logprobs`` / ``top_logprobs=k``: ``pool.last_logprobs[stream]``, ``pool.last_top_ids[stream]`` /
        ``pool.last_top_logprobs[stream]`` of a stream's latest caption, cut the same way; ``pool.last_frames[stream]`` = the frames
        it saw.  ``pool.caption(streams)`` captions now, ``pool.drop(stream)`` empties one stream, ``pool.counts()`` = frames held
        per stream.  Camera frames need the native encoder; memory tokens [n, d_model] can be pushed without one.
        The pool and a caption_stream() of the same model live side by side: opening one does not invalidate the other.  Opening
        another pool, moving the model or loading weights invalidates this one.
        Out of scope: scene-change gates (put one FrameGate per camera in front of ``push``; deciding all cameras' gates in one
        launch is a later change) and ``carry`` / drafts.
        ``beams=k`` (include/gitcap.h: gitcap_student_pool_beam_search): the due cameras are captioned by beam search, max_batch // k
        of them per call, the k beam rows of a camera reading its K|V rows through the key tables (nothing is repeated).  A caption is
        then the best beam [max_len] (not cut; max_len counts CLS, as in beam_search), bit for bit beam_search(max_len, k) on a list
        holding the camera's frames.  With ``eos=True`` (and length_penalty / num_keep_best / per_node_beam_size /
        repetition_penalty, as in beam_search) it is rank 0 of the search that ends hypotheses at SEP, ``pool.last_scores[stream]``
        [n] holds its scores and ``pool.last_predictions[stream]`` [n, max_len] / ``pool.last_lengths[stream]`` [n] all ranks.  One
        set of search rules for every camera; log-probabilities and alternatives belong to the greedy pool.
        no_repeat_ngram_size / min_length / suppress_tokens (as in greedy_decode): one set of rules for every camera's captions,
        attached again for every pool call; rules per camera are out of scope.
        ``pool.set_prompt(stream, ids)``: a standing text prefix for one camera (ids 1-D, CLS prepended where missing; None removes
        it), kept until replaced; every pool call attaches the ragged table of the cameras it captions, and a camera's caption is
        greedy_decode(prompt=[ids]) on its frames.  ``pool.last_prompt_lengths[stream]`` = the prompt tokens of its latest caption."""
        if not 0 <= int(top_logprobs) <= 32:
            raise ValueError(f"top_logprobs={top_logprobs} outside 0..32")
        if streams < 1 or streams > 4096:
            raise ValueError(f"streams={streams} outside 1..4096")
        mode = {"all_sep": STOP_ALL_SEP, "never": STOP_NEVER}[stop or self.stop]
        if beams is None:
            if eos or length_penalty != 1.0 or num_keep_best != 1 or per_node_beam_size is not None or repetition_penalty != 1.0:
                raise ValueError("eos= and the search arguments are for pools with beams")
            if max_len < 1 or max_len > self.max_text_len:
                raise ValueError(f"max_len={max_len} outside 1..max_text_len={self.max_text_len}")
            co = self._constraints(no_repeat_ngram_size, min_length, suppress_tokens, max_len)
            return StudentStreamPool(self, streams, hop, max_len, mode, logprobs, top_logprobs, min_frames, co)
        if logprobs or top_logprobs:
            raise ValueError("logprobs / top_logprobs are for greedy pools: they cannot be combined with beams")
        if max_len < 2 or max_len - 1 > self.max_text_len or beams < 1 or beams > min(16, self.max_batch):
            raise ValueError(f"a pool with beams needs 2 <= max_len <= max_text_len+1={self.max_text_len + 1} and 1 <= beams <= min(16, max_batch)")
        se = _search_options(eos, beams, length_penalty, num_keep_best, per_node_beam_size, repetition_penalty)
        co = self._constraints(no_repeat_ngram_size, min_length, suppress_tokens, max_len, beams if se is None else beams * se.pn)
        return StudentStreamPool(self, streams, hop, max_len, mode, False, 0, min_frames, co, beams, se)

    @torch.no_grad()
    def beam_search_host(self, src: torch.Tensor, max_len: int = 10, k: int = 3, no_repeat_ngram_size: int = 0, min_length: int = 0,
                         suppress_tokens=None, prompt=None, prompt_lengths=None, eos: bool = False, length_penalty: float = 1.0,
                         num_keep_best: int = 1, per_node_beam_size: Optional[int] = None, repetition_penalty: float = 1.0,
                         frame_counts=None, stats: Optional[dict] = None):
        """The same search driven from the host the way the reference writes it (every step recomputes the whole prefix
        through ``forward_decoder``, one host sync per step): the cross-check of ``beam_search`` in the tests.  The constraint
        arguments (as in beam_search) set every row's banned logits to -inf ahead of the log_softmax.
        prompt / prompt_lengths (as in beam_search): the search of every clip starts from its own prefix instead of the lone CLS;
        prompts of different lengths are searched clip by clip (the reference's loop advances all rows in lockstep).
        ``eos=True`` and the search arguments (as in beam_search): gitcap.search.eos_beam_search -- the teacher's search operator as
        host logic -- over ``forward_decoder`` on the growing prefix: the yardstick of beam_search(eos=True), with its dict plus
        ``last_tokens`` [B, n], the candidate that finished each hypothesis.  This form also takes frame_counts (or ``src`` as a
        list of clips) and fills ``stats`` (eos_beam_search's)."""
        from .search import banned_tokens, check_constraints, eos_beam_search
        cn, cm, sup = check_constraints(no_repeat_ngram_size, min_length, suppress_tokens)
        V, sep = self.cfg.vocab_length, self.cfg.sep_token_id

        def rule(logits, prefixes):         # logits [rows, V] of the rows whose ids so far are prefixes [rows, L]
            if not (cn or cm or sup):
                return logits
            logits = logits.clone()
            for r, pre in enumerate(prefixes.tolist()):
                cols = banned_tokens(pre, cn, cm, sep, sup, V)
                if cols:
                    logits[r, cols] = float("-inf")
            return logits

        se = _search_options(eos, k, length_penalty, num_keep_best, per_node_beam_size, repetition_penalty)
        if se is not None:
            if self._is_ragged(src, frame_counts):
                mems, _, out_dev = self._clip_memories(src, frame_counts)
            else:
                out_dev = src.device
                mems = list(self._memory(self._src_memory(src)))
            B = len(mems)
            if B * k > self.max_batch or max_len - 1 > self.max_text_len or max_len < 2:
                raise ValueError(f"B*k={B * k} rows > max_batch={self.max_batch}, or max_len={max_len} outside 2..max_text_len+1")
            pr = self._prompt(prompt, prompt_lengths, B, max_len - 1, "max_len - 1")
            start = [[self.cls_token_id]] * B if pr is None else [pr.ids[b, :n].tolist() for b, n in enumerate(pr.host_lengths)]
            mem_rep = [m for m in mems for _ in range(k)]                               # row b*k + i = beam i of clip b
            res = eos_beam_search(lambda ids: self.forward_decoder(ids, mem_rep)[:, -1].cpu(), start, k=k, max_len=max_len, sep_id=sep,
                                  length_penalty=se.lp, num_keep_best=se.n, per_node_beam_size=se.pn, repetition_penalty=se.rp,
                                  rule=rule, stats=stats)
            return {name: t.to(out_dev) for name, t in res.items()}
        out_dev = src.device
        memory = self._src_memory(src)
        mem = self._memory(memory)
        B = mem.shape[0]
        if B * k > self.max_batch:
            raise ValueError(f"B*k={B * k} rows > max_batch={self.max_batch}")
        if max_len - 1 > self.max_text_len:
            raise ValueError(f"max_len={max_len} exceeds max_text_len+1={self.max_text_len + 1}")
        pr = self._prompt(prompt, prompt_lengths, B, max_len - 1, "max_len - 1")
        if pr is not None and pr.min_len != pr.max_len:
            rows = [self.beam_search_host(mem[b:b + 1], max_len, k, no_repeat_ngram_size, min_length, suppress_tokens,
                                          prompt=pr.ids[b:b + 1, :pr.host_lengths[b]]) for b in range(B)]
            best = torch.cat(rows, 0)
            return best.to(out_dev) if out_dev != best.device else best
        tgt = torch.full((B, 1), self.cls_token_id, dtype=torch.long, device=self._dev) if pr is None else pr.ids[:, :pr.max_len]
        logp = torch.log_softmax(rule(self.forward_decoder(tgt, mem)[:, -1], tgt), dim=-1)  # model.py:221-225
        scores, top = logp.topk(k, dim=-1)
        seqs = torch.cat([tgt.unsqueeze(1).expand(-1, k, -1), top.unsqueeze(-1)], dim=-1)  # [B, k, 2] (a prompt: [B, k, P + 1])
        mem_rep = mem.repeat_interleave(k, dim=0)                                          # row b*k + i = beam i of clip b
        for _ in range(tgt.shape[1] + 1, max_len):                                         # model.py:230
            rows = seqs.reshape(B * k, -1)
            lp = torch.log_softmax(rule(self.forward_decoder(rows, mem_rep)[:, -1], rows), dim=-1)
            ts, ti = lp.view(B, k, -1).topk(k, dim=-1)                                     # each beam's top-k
            cand = (scores.unsqueeze(-1) + ts).view(B, k * k)                              # beam-major, as all_candidates
            sel = cand.sort(dim=1, descending=True).indices[:, :k]                         # model.py:252-256
            beam = sel // k
            seqs = torch.cat([seqs.gather(1, beam.unsqueeze(-1).expand(-1, -1, seqs.shape[-1])),
                              ti.view(B, k * k).gather(1, sel).unsqueeze(-1)], dim=-1)
            scores = cand.gather(1, sel)
        best = seqs[torch.arange(B, device=self._dev), scores.argmax(dim=-1)]              # model.py:317
        return best.to(out_dev) if out_dev != best.device else best
