"""Status code and exact *_last_error text of every argument check and state check of the greedy and beam entry points of the
teacher (gitcap_greedy, _raw, _submit, _raw_submit, gitcap_beam_search, _submit, _raw_submit, gitcap_window_greedy,
gitcap_window_beam_search) and of the student (gitcap_student_greedy, _window_greedy, _greedy_draft, _window_greedy_draft), on
git_tiny(2) and the tiny student.

The entry points of a family run one shared body; what differs between them (the synchronous raw path does not run the raw-frame
checks the submitted one runs, the window forms check the window behind the arguments) is pinned here as recorded behaviour.  The
tables were recorded on the commit before the entry points were folded.  No arithmetic: a refused call launches nothing.  The
"sizes overflow" case is driven through the submitted raw paths only: the synchronous raw path has no such check and would launch.

An attachment (gitcap_attach_token_logprobs and its student twin) is consumed by a call that then fails its argument check."""
import ctypes

import pytest
import torch

from gitcap.config import git_tiny
from gitcap.student_config import student_synthetic_weights, student_tiny
from gitcap.weights import synthetic_weights
from gpu_support import camera, stream
from oracle.git_oracle import make_frames
from oracle.student_oracle import make_memory

pytestmark = pytest.mark.gpu

L = 8            # max_text_len of both handles
POISON = -4321.0


def _p(t, off=0):
    """gpu_support.ptr with a byte offset: the misaligned buffers the entry points must refuse"""
    return ctypes.c_void_p(t.data_ptr() + off) if t is not None else None


# ---- teacher ---------------------------------------------------------------------------------------------------------------------

GREEDY = ("gitcap_greedy", "gitcap_greedy_raw", "gitcap_greedy_submit", "gitcap_greedy_raw_submit")
BEAM = ("gitcap_beam_search", "gitcap_beam_search_submit", "gitcap_beam_search_raw_submit")


class _Teacher:
    def __init__(self, weights=True):
        from gitcap.model import GitCaptioner
        cfg = git_tiny(2)
        self.m = GitCaptioner(cfg, synthetic_weights(cfg, 0) if weights else None, max_batch=2, max_frames=2, max_text_len=L,
                              max_beams=2, stop="never")
        self.lib, self.h = self.m._lib, self.m._handle
        self.f32 = make_frames(2, 2, cfg.image_size, 1234).cuda()
        self.u8 = camera((2, 2, 80, 96, 3), 5).cuda()
        self.ids = torch.full((2, L + 1), -1, dtype=torch.int64, device="cuda")
        self.steps = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.dec = torch.zeros((2, 16), dtype=torch.int64, device="cuda")
        self.blp = torch.zeros((2, 16), device="cuda")
        self.lp = torch.full((2, L), POISON, device="cuda")
        self.vis = torch.zeros(64, device="cuda")
        self.rows = []

    def rec(self, label, rc, h=True):
        e = self.lib.gitcap_last_error(self.h if h else None)
        self.rows.append((label, rc, (e or b"").decode()))

    def attach(self, ld):
        assert self.lib.gitcap_attach_token_logprobs(self.h, _p(self.lp), ld) == 0

    def greedy(self, name, h=True, src="own", B=2, F=2, H=80, W=96, max_len=L, stop=0, ids="own", ticket=True):
        raw, sub = "raw" in name, "submit" in name
        src = (_p(self.u8) if raw else _p(self.f32)) if src == "own" else src
        tk = ctypes.c_int(-1)
        args = [self.h if h else None, src, B, F] + ([H, W] if raw else []) + [max_len, stop, _p(self.ids) if ids == "own" else ids,
                                                                              _p(self.steps), stream()]
        rc = getattr(self.lib, name)(*args, *([ctypes.byref(tk) if ticket else None] if sub else []))
        if sub and rc == 0:
            assert self.lib.gitcap_greedy_wait(self.h, tk.value, stream()) == 0
        return rc

    def beam(self, name, h=True, src="own", B=2, F=2, H=80, W=96, beams=2, steps=L, pnb=2, dec="own", blp="own", ticket=True):
        raw, sub = "raw" in name, "submit" in name
        src = (_p(self.u8) if raw else _p(self.f32)) if src == "own" else src
        tk = ctypes.c_int(-1)
        args = [self.h if h else None, src, B, F] + ([H, W] if raw else []) + ([None] if sub else [])
        args += [beams, steps, 1.0, pnb, _p(self.dec) if dec == "own" else dec, _p(self.blp) if blp == "own" else blp]
        args += ([None] if sub else []) + [stream()] + ([ctypes.byref(tk) if ticket else None] if sub else [])
        return getattr(self.lib, name)(*args)

    def window_greedy(self, h=True, max_len=L, stop=0, vis=None, ids="own"):
        return self.lib.gitcap_window_greedy(self.h if h else None, max_len, stop, vis, _p(self.ids) if ids == "own" else ids,
                                             _p(self.steps), stream())

    def window_beam(self, h=True, beams=2, steps=L, pnb=2, vis=None, dec="own"):
        return self.lib.gitcap_window_beam_search(self.h if h else None, beams, steps, 1.0, pnb, vis,
                                                  _p(self.dec) if dec == "own" else dec, _p(self.blp), stream())


def _teacher_observed():
    t = _Teacher()
    for name in GREEDY:
        g = lambda **kw: t.greedy(name, **kw)                                       # noqa: E731
        t.rec(f"{name}: null handle", g(h=False), h=False)
        if "submit" in name:
            t.rec(f"{name}: null ticket", g(ticket=False))
        t.rec(f"{name}: null ids_out", g(ids=None))
        t.rec(f"{name}: max_len 0", g(max_len=0))
        t.rec(f"{name}: max_len 9", g(max_len=L + 1))
        t.rec(f"{name}: stop 7", g(stop=7))
        t.attach(L - 1)
        t.rec(f"{name}: attached ld 7", g())
        t.attach(L - 1)
        t.rec(f"{name}: attached ld 7 and stop 7", g(stop=7))
        t.rec(f"{name}: B 3", g(B=3))
        t.rec(f"{name}: F 3", g(F=3))
        t.rec(f"{name}: B 0", g(B=0))
        t.rec(f"{name}: null frames", g(src=None))
        if "raw" in name:
            t.rec(f"{name}: H 0", g(H=0))
            t.rec(f"{name}: W 0", g(W=0))
            if "submit" in name:
                t.rec(f"{name}: sizes overflow", g(H=1 << 19, W=1 << 19))
        else:
            t.rec(f"{name}: misaligned frames", g(src=_p(t.f32, 4)))
        # consumed by a call that fails its argument check: the valid call behind it leaves the buffer alone
        t.lp.fill_(POISON)
        t.attach(L)
        t.rec(f"{name}: attached, null ids_out", g(ids=None))
        rc = g()
        torch.cuda.synchronize()
        t.rec(f"{name}: valid call, attachment untouched={bool((t.lp == POISON).all())}", rc)
    for name in BEAM:
        b = lambda **kw: t.beam(name, **kw)                                         # noqa: E731
        t.rec(f"{name}: null handle", b(h=False), h=False)
        if "submit" in name:
            t.rec(f"{name}: null ticket", b(ticket=False))
        t.rec(f"{name}: null decoded_out", b(dec=None))
        t.rec(f"{name}: null logprobs_out", b(blp=None))
        t.rec(f"{name}: beams 0", b(beams=0))
        t.rec(f"{name}: per_node_beam_size 0", b(pnb=0))
        t.rec(f"{name}: beams 3", b(beams=3))
        t.rec(f"{name}: beams 2 x 9 candidates", b(pnb=9))
        t.rec(f"{name}: max_steps 1", b(steps=1))
        t.rec(f"{name}: max_steps 9", b(steps=L + 1))
        t.rec(f"{name}: per_node_beam_size 1", b(pnb=1))
        t.rec(f"{name}: B 3", b(B=3))
        t.rec(f"{name}: F 3", b(F=3))
        t.rec(f"{name}: null frames", b(src=None))
        if "raw" in name:
            t.rec(f"{name}: H 0", b(H=0))
            t.rec(f"{name}: W 0", b(W=0))
            t.rec(f"{name}: sizes overflow", b(H=1 << 19, W=1 << 19))
        else:
            t.rec(f"{name}: misaligned frames", b(src=_p(t.f32, 4)))
    # the window forms: the family's argument checks, then the window's state
    t.rec("gitcap_window_greedy: null handle", t.window_greedy(h=False), h=False)
    t.rec("gitcap_window_greedy: no window", t.window_greedy())
    t.rec("gitcap_window_greedy: no window, null ids_out", t.window_greedy(ids=None))
    t.rec("gitcap_window_greedy: max_len 0", t.window_greedy(max_len=0))
    t.rec("gitcap_window_greedy: max_len 9", t.window_greedy(max_len=L + 1))
    t.rec("gitcap_window_greedy: stop 7", t.window_greedy(stop=7))
    t.attach(L - 1)
    t.rec("gitcap_window_greedy: attached ld 7", t.window_greedy())
    t.rec("gitcap_window_beam_search: null handle", t.window_beam(h=False), h=False)
    t.rec("gitcap_window_beam_search: no window", t.window_beam())
    t.rec("gitcap_window_beam_search: no window, null decoded_out", t.window_beam(dec=None))
    t.rec("gitcap_window_beam_search: beams 3", t.window_beam(beams=3))
    t.rec("gitcap_window_beam_search: max_steps 9", t.window_beam(steps=L + 1))
    assert t.lib.gitcap_window_reset(t.h, 2, 2) == 0
    t.rec("gitcap_window_greedy: empty window", t.window_greedy())
    t.rec("gitcap_window_beam_search: empty window", t.window_beam())
    one = t.f32[:, :1].contiguous()
    assert t.lib.gitcap_window_push(t.h, _p(one), 2, 1, stream()) == 0
    t.rec("gitcap_window_greedy: 1 of 2 frames", t.window_greedy())
    t.rec("gitcap_window_beam_search: 1 of 2 frames", t.window_beam())
    assert t.lib.gitcap_window_push(t.h, _p(one), 2, 1, stream()) == 0
    t.rec("gitcap_window_greedy: misaligned visual_out", t.window_greedy(vis=_p(t.vis, 4)))
    t.rec("gitcap_window_beam_search: misaligned visual_out", t.window_beam(vis=_p(t.vis, 4)))
    t.lp.fill_(POISON)
    t.attach(L)
    t.rec("gitcap_window_greedy: attached, stop 7", t.window_greedy(stop=7))
    rc = t.window_greedy()
    torch.cuda.synchronize()
    t.rec(f"gitcap_window_greedy: valid call, attachment untouched={bool((t.lp == POISON).all())}", rc)
    # before gitcap_finalize_weights
    u = _Teacher(weights=False)
    for name in GREEDY:
        u.rec(f"{name}: not finalized", u.greedy(name))
        u.rec(f"{name}: not finalized, stop 7", u.greedy(name, stop=7))
    for name in BEAM:
        u.rec(f"{name}: not finalized", u.beam(name))
    u.rec("gitcap_window_greedy: not finalized", u.window_greedy())
    u.rec("gitcap_window_beam_search: not finalized", u.window_beam())
    torch.cuda.synchronize()
    return t.rows + u.rows


# ---- student ---------------------------------------------------------------------------------------------------------------------

S_LEN = 6
STUDENT = ("gitcap_student_greedy", "gitcap_student_window_greedy", "gitcap_student_greedy_draft", "gitcap_student_window_greedy_draft")


class _Student:
    def __init__(self, weights=True):
        from gitcap.student import StudentCaptioner
        cfg = self.cfg = student_tiny()
        self.m = StudentCaptioner(cfg=cfg, weights=student_synthetic_weights(cfg, 0) if weights else None, device="cuda:0",
                                  max_batch=2, max_text_len=L)
        self.lib, self.h = self.m._lib, self.m._handle
        self.mem = make_memory(2, cfg.mem_tokens, cfg.d_model, 5).cuda()
        self.d = torch.full((2, S_LEN + 1), 3, dtype=torch.int64, device="cuda")
        self.ids = torch.full((2, S_LEN + 1), -1, dtype=torch.int64, device="cuda")
        self.steps = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.lp = torch.full((2, S_LEN), POISON, device="cuda")
        self.rows = []

    def rec(self, label, rc, h=True):
        e = self.lib.gitcap_student_last_error(self.h if h else None)
        self.rows.append((label, rc, (e or b"").decode()))

    def attach(self, ld):
        assert self.lib.gitcap_student_attach_token_logprobs(self.h, _p(self.lp), ld) == 0

    def call(self, name, h=True, mem="own", B=2, d="own", ld=S_LEN + 1, n=S_LEN, max_len=S_LEN, stop=0, ids="own"):
        args = [self.h if h else None]
        if "window" not in name:
            args += [_p(self.mem) if mem == "own" else mem, B]
        if "draft" in name:
            args += [_p(self.d) if d == "own" else d, ld, n]
        args += [max_len, stop, _p(self.ids) if ids == "own" else ids, _p(self.steps)]
        if "draft" in name:
            args += [None]
        return getattr(self.lib, name)(*args, stream())


def _student_observed():
    t = _Student()
    F = t.cfg.mem_tokens

    def checks(name, state):
        c = lambda **kw: t.call(name, **kw)                                         # noqa: E731
        t.rec(f"{name} [{state}]: null ids_out", c(ids=None))
        t.rec(f"{name} [{state}]: max_len 0", c(max_len=0))
        t.rec(f"{name} [{state}]: max_len 9", c(max_len=L + 1, n=2))
        t.rec(f"{name} [{state}]: stop 7", c(stop=7))
        t.attach(S_LEN - 1)
        t.rec(f"{name} [{state}]: attached ld 5", c())
        t.attach(S_LEN - 1)
        t.rec(f"{name} [{state}]: attached ld 5 and stop 7", c(stop=7))
        if "draft" in name:
            t.rec(f"{name} [{state}]: null draft_ids", c(d=None))
            t.rec(f"{name} [{state}]: n_draft 0", c(n=0))
            t.rec(f"{name} [{state}]: n_draft 7", c(n=S_LEN + 1, ld=S_LEN + 2))
            t.rec(f"{name} [{state}]: ld_draft 6", c(ld=S_LEN))
            t.attach(S_LEN - 1)
            t.rec(f"{name} [{state}]: attached ld 5 and null draft_ids", c(d=None))
        if "window" not in name:
            t.rec(f"{name} [{state}]: null memory", c(mem=None))
            t.rec(f"{name} [{state}]: B 0", c(B=0))
            t.rec(f"{name} [{state}]: B 3", c(B=3))

    for name in STUDENT:
        t.rec(f"{name}: null handle", t.call(name, h=False), h=False)
        checks(name, "no window")
        if "window" in name:
            t.rec(f"{name}: no window", t.call(name))
    assert t.lib.gitcap_student_window_reset(t.h, 2) == 0
    for name in STUDENT[1::2]:
        t.rec(f"{name}: empty window", t.call(name))
    part = t.mem[:, :F - 1].contiguous()
    assert t.lib.gitcap_student_window_push(t.h, _p(part), 2, F - 1, stream()) == 0
    for name in STUDENT[1::2]:
        t.rec(f"{name}: F - 1 tokens", t.call(name))
        t.rec(f"{name}: F - 1 tokens, stop 7", t.call(name, stop=7))
    t.rec("gitcap_student_window_greedy_draft: F - 1 tokens, n_draft 0", t.call(STUDENT[3], n=0))
    assert t.lib.gitcap_student_window_push(t.h, _p(t.mem[:, F - 1:].contiguous()), 2, 1, stream()) == 0
    for name in STUDENT:
        if "window" in name:
            checks(name, "full window")
        # consumed by a call that fails its argument check: the valid call behind it leaves the buffer alone
        t.lp.fill_(POISON)
        t.attach(S_LEN)
        t.rec(f"{name}: attached, null ids_out", t.call(name, ids=None))
        rc = t.call(name)
        torch.cuda.synchronize()
        t.rec(f"{name}: valid call, attachment untouched={bool((t.lp == POISON).all())}", rc)
    # before gitcap_student_finalize
    u = _Student(weights=False)
    u.rec("gitcap_student_attach_token_logprobs: not finalized", u.lib.gitcap_student_attach_token_logprobs(u.h, _p(u.lp), S_LEN))
    for name in STUDENT:
        u.rec(f"{name}: not finalized", u.call(name))
        u.rec(f"{name}: not finalized, stop 7", u.call(name, stop=7))
    assert u.lib.gitcap_student_window_reset(u.h, 2) == 0
    for name in STUDENT[1::2]:
        u.rec(f"{name}: not finalized, empty window", u.call(name))
    torch.cuda.synchronize()
    return t.rows + u.rows


TEACHER_EXPECTED = [
    ('gitcap_greedy: null handle', -1, 'greedy: null handle'),
    ('gitcap_greedy: null ids_out', -1, 'greedy: bad arguments'),
    ('gitcap_greedy: max_len 0', -1, 'greedy: bad arguments'),
    ('gitcap_greedy: max_len 9', -1, 'greedy: max_len exceeds max_text_len'),
    ('gitcap_greedy: stop 7', -1, 'greedy: unknown stop rule'),
    ('gitcap_greedy: attached ld 7', -1, 'greedy: the attached token log-probability buffer has ld < max_len'),
    ('gitcap_greedy: attached ld 7 and stop 7', -1, 'greedy: unknown stop rule'),
    ('gitcap_greedy: B 3', -1, 'encode: B/F exceed the sizes the handle was created for'),
    ('gitcap_greedy: F 3', -1, 'encode: B/F exceed the sizes the handle was created for'),
    ('gitcap_greedy: B 0', -1, 'encode: bad arguments'),
    ('gitcap_greedy: null frames', -1, 'encode: bad arguments'),
    ('gitcap_greedy: misaligned frames', -1, 'encode: frames must be 16-byte aligned'),
    ('gitcap_greedy: attached, null ids_out', -1, 'greedy: bad arguments'),
    ('gitcap_greedy: valid call, attachment untouched=True', 0, 'greedy: bad arguments'),
    ('gitcap_greedy_raw: null handle', -1, 'greedy_raw: null handle'),
    ('gitcap_greedy_raw: null ids_out', -1, 'greedy: bad arguments'),
    ('gitcap_greedy_raw: max_len 0', -1, 'greedy: bad arguments'),
    ('gitcap_greedy_raw: max_len 9', -1, 'greedy: max_len exceeds max_text_len'),
    ('gitcap_greedy_raw: stop 7', -1, 'greedy: unknown stop rule'),
    ('gitcap_greedy_raw: attached ld 7', -1, 'greedy: the attached token log-probability buffer has ld < max_len'),
    ('gitcap_greedy_raw: attached ld 7 and stop 7', -1, 'greedy: unknown stop rule'),
    ('gitcap_greedy_raw: B 3', -1, 'encode: B/F exceed the sizes the handle was created for'),
    ('gitcap_greedy_raw: F 3', -1, 'encode: B/F exceed the sizes the handle was created for'),
    ('gitcap_greedy_raw: B 0', -1, 'encode: bad arguments'),
    ('gitcap_greedy_raw: null frames', -1, 'encode: bad arguments'),
    ('gitcap_greedy_raw: H 0', -1, 'encode_raw: frames smaller than the crop, or bad sizes'),
    ('gitcap_greedy_raw: W 0', -1, 'encode_raw: frames smaller than the crop, or bad sizes'),
    ('gitcap_greedy_raw: attached, null ids_out', -1, 'greedy: bad arguments'),
    ('gitcap_greedy_raw: valid call, attachment untouched=True', 0, 'greedy: bad arguments'),
    ('gitcap_greedy_submit: null handle', -1, 'greedy_submit: null argument'),
    ('gitcap_greedy_submit: null ticket', -1, 'greedy_submit: null argument'),
    ('gitcap_greedy_submit: null ids_out', -1, 'greedy: bad arguments'),
    ('gitcap_greedy_submit: max_len 0', -1, 'greedy: bad arguments'),
    ('gitcap_greedy_submit: max_len 9', -1, 'greedy: max_len exceeds max_text_len'),
    ('gitcap_greedy_submit: stop 7', -1, 'greedy: unknown stop rule'),
    ('gitcap_greedy_submit: attached ld 7', -1, 'greedy: the attached token log-probability buffer has ld < max_len'),
    ('gitcap_greedy_submit: attached ld 7 and stop 7', -1, 'greedy: unknown stop rule'),
    ('gitcap_greedy_submit: B 3', -1, 'encode: B/F exceed the sizes the handle was created for'),
    ('gitcap_greedy_submit: F 3', -1, 'encode: B/F exceed the sizes the handle was created for'),
    ('gitcap_greedy_submit: B 0', -1, 'encode: bad arguments'),
    ('gitcap_greedy_submit: null frames', -1, 'encode: bad arguments'),
    ('gitcap_greedy_submit: misaligned frames', -1, 'encode: frames must be 16-byte aligned'),
    ('gitcap_greedy_submit: attached, null ids_out', -1, 'greedy: bad arguments'),
    ('gitcap_greedy_submit: valid call, attachment untouched=True', 0, 'greedy: bad arguments'),
    ('gitcap_greedy_raw_submit: null handle', -1, 'greedy_raw_submit: null argument'),
    ('gitcap_greedy_raw_submit: null ticket', -1, 'greedy_raw_submit: null argument'),
    ('gitcap_greedy_raw_submit: null ids_out', -1, 'greedy: bad arguments'),
    ('gitcap_greedy_raw_submit: max_len 0', -1, 'greedy: bad arguments'),
    ('gitcap_greedy_raw_submit: max_len 9', -1, 'greedy: max_len exceeds max_text_len'),
    ('gitcap_greedy_raw_submit: stop 7', -1, 'greedy: unknown stop rule'),
    ('gitcap_greedy_raw_submit: attached ld 7', -1, 'greedy: the attached token log-probability buffer has ld < max_len'),
    ('gitcap_greedy_raw_submit: attached ld 7 and stop 7', -1, 'greedy: unknown stop rule'),
    ('gitcap_greedy_raw_submit: B 3', -1, 'encode: B/F exceed the sizes the handle was created for'),
    ('gitcap_greedy_raw_submit: F 3', -1, 'encode: B/F exceed the sizes the handle was created for'),
    ('gitcap_greedy_raw_submit: B 0', -1, 'encode: bad arguments'),
    ('gitcap_greedy_raw_submit: null frames', -1, 'raw frames: null pointer or empty frames'),
    ('gitcap_greedy_raw_submit: H 0', -1, 'raw frames: null pointer or empty frames'),
    ('gitcap_greedy_raw_submit: W 0', -1, 'raw frames: null pointer or empty frames'),
    ('gitcap_greedy_raw_submit: sizes overflow', -1, 'raw frames: sizes overflow'),
    ('gitcap_greedy_raw_submit: attached, null ids_out', -1, 'greedy: bad arguments'),
    ('gitcap_greedy_raw_submit: valid call, attachment untouched=True', 0, 'greedy: bad arguments'),
    ('gitcap_beam_search: null handle', -1, 'beam_search: null handle'),
    ('gitcap_beam_search: null decoded_out', -1, 'beam_search: bad arguments'),
    ('gitcap_beam_search: null logprobs_out', -1, 'beam_search: bad arguments'),
    ('gitcap_beam_search: beams 0', -1, 'beam_search: bad arguments'),
    ('gitcap_beam_search: per_node_beam_size 0', -1, 'beam_search: bad arguments'),
    ('gitcap_beam_search: beams 3', -1, 'beam_search: beams exceed max_beams / 16 candidates'),
    ('gitcap_beam_search: beams 2 x 9 candidates', -1, 'beam_search: beams exceed max_beams / 16 candidates'),
    ('gitcap_beam_search: max_steps 1', -1, 'beam_search: max_steps outside [2, max_text_len]'),
    ('gitcap_beam_search: max_steps 9', -1, 'beam_search: max_steps outside [2, max_text_len]'),
    ('gitcap_beam_search: per_node_beam_size 1', -1, 'beam_search: per_node_beam_size must be >= 2 (model.py:606)'),
    ('gitcap_beam_search: B 3', -1, 'encode: B/F exceed the sizes the handle was created for'),
    ('gitcap_beam_search: F 3', -1, 'encode: B/F exceed the sizes the handle was created for'),
    ('gitcap_beam_search: null frames', -1, 'encode: bad arguments'),
    ('gitcap_beam_search: misaligned frames', -1, 'encode: frames must be 16-byte aligned'),
    ('gitcap_beam_search_submit: null handle', -1, 'beam_search_submit: null argument'),
    ('gitcap_beam_search_submit: null ticket', -1, 'beam_search_submit: null argument'),
    ('gitcap_beam_search_submit: null decoded_out', -1, 'beam_search: bad arguments'),
    ('gitcap_beam_search_submit: null logprobs_out', -1, 'beam_search: bad arguments'),
    ('gitcap_beam_search_submit: beams 0', -1, 'beam_search: bad arguments'),
    ('gitcap_beam_search_submit: per_node_beam_size 0', -1, 'beam_search: bad arguments'),
    ('gitcap_beam_search_submit: beams 3', -1, 'beam_search: beams exceed max_beams / 16 candidates'),
    ('gitcap_beam_search_submit: beams 2 x 9 candidates', -1, 'beam_search: beams exceed max_beams / 16 candidates'),
    ('gitcap_beam_search_submit: max_steps 1', -1, 'beam_search: max_steps outside [2, max_text_len]'),
    ('gitcap_beam_search_submit: max_steps 9', -1, 'beam_search: max_steps outside [2, max_text_len]'),
    ('gitcap_beam_search_submit: per_node_beam_size 1', -1, 'beam_search: per_node_beam_size must be >= 2 (model.py:606)'),
    ('gitcap_beam_search_submit: B 3', -1, 'encode: B/F exceed the sizes the handle was created for'),
    ('gitcap_beam_search_submit: F 3', -1, 'encode: B/F exceed the sizes the handle was created for'),
    ('gitcap_beam_search_submit: null frames', -1, 'encode: bad arguments'),
    ('gitcap_beam_search_submit: misaligned frames', -1, 'encode: frames must be 16-byte aligned'),
    ('gitcap_beam_search_raw_submit: null handle', -1, 'beam_search_raw_submit: null argument'),
    ('gitcap_beam_search_raw_submit: null ticket', -1, 'beam_search_raw_submit: null argument'),
    ('gitcap_beam_search_raw_submit: null decoded_out', -1, 'beam_search: bad arguments'),
    ('gitcap_beam_search_raw_submit: null logprobs_out', -1, 'beam_search: bad arguments'),
    ('gitcap_beam_search_raw_submit: beams 0', -1, 'beam_search: bad arguments'),
    ('gitcap_beam_search_raw_submit: per_node_beam_size 0', -1, 'beam_search: bad arguments'),
    ('gitcap_beam_search_raw_submit: beams 3', -1, 'beam_search: beams exceed max_beams / 16 candidates'),
    ('gitcap_beam_search_raw_submit: beams 2 x 9 candidates', -1, 'beam_search: beams exceed max_beams / 16 candidates'),
    ('gitcap_beam_search_raw_submit: max_steps 1', -1, 'beam_search: max_steps outside [2, max_text_len]'),
    ('gitcap_beam_search_raw_submit: max_steps 9', -1, 'beam_search: max_steps outside [2, max_text_len]'),
    ('gitcap_beam_search_raw_submit: per_node_beam_size 1', -1, 'beam_search: per_node_beam_size must be >= 2 (model.py:606)'),
    ('gitcap_beam_search_raw_submit: B 3', -1, 'encode: B/F exceed the sizes the handle was created for'),
    ('gitcap_beam_search_raw_submit: F 3', -1, 'encode: B/F exceed the sizes the handle was created for'),
    ('gitcap_beam_search_raw_submit: null frames', -1, 'raw frames: null pointer or empty frames'),
    ('gitcap_beam_search_raw_submit: H 0', -1, 'raw frames: null pointer or empty frames'),
    ('gitcap_beam_search_raw_submit: W 0', -1, 'raw frames: null pointer or empty frames'),
    ('gitcap_beam_search_raw_submit: sizes overflow', -1, 'raw frames: sizes overflow'),
    ('gitcap_window_greedy: null handle', -1, 'window_greedy: null handle'),
    ('gitcap_window_greedy: no window', -2, 'window: fewer than F frames pushed since the reset'),
    ('gitcap_window_greedy: no window, null ids_out', -1, 'greedy: bad arguments'),
    ('gitcap_window_greedy: max_len 0', -1, 'greedy: bad arguments'),
    ('gitcap_window_greedy: max_len 9', -1, 'greedy: max_len exceeds max_text_len'),
    ('gitcap_window_greedy: stop 7', -1, 'greedy: unknown stop rule'),
    ('gitcap_window_greedy: attached ld 7', -1, 'greedy: the attached token log-probability buffer has ld < max_len'),
    ('gitcap_window_beam_search: null handle', -1, 'window_beam_search: null handle'),
    ('gitcap_window_beam_search: no window', -2, 'window: fewer than F frames pushed since the reset'),
    ('gitcap_window_beam_search: no window, null decoded_out', -1, 'beam_search: bad arguments'),
    ('gitcap_window_beam_search: beams 3', -1, 'beam_search: beams exceed max_beams / 16 candidates'),
    ('gitcap_window_beam_search: max_steps 9', -1, 'beam_search: max_steps outside [2, max_text_len]'),
    ('gitcap_window_greedy: empty window', -2, 'window: fewer than F frames pushed since the reset'),
    ('gitcap_window_beam_search: empty window', -2, 'window: fewer than F frames pushed since the reset'),
    ('gitcap_window_greedy: 1 of 2 frames', -2, 'window: fewer than F frames pushed since the reset'),
    ('gitcap_window_beam_search: 1 of 2 frames', -2, 'window: fewer than F frames pushed since the reset'),
    ('gitcap_window_greedy: misaligned visual_out', -1, 'window: visual_out must be 16-byte aligned'),
    ('gitcap_window_beam_search: misaligned visual_out', -1, 'window: visual_out must be 16-byte aligned'),
    ('gitcap_window_greedy: attached, stop 7', -1, 'greedy: unknown stop rule'),
    ('gitcap_window_greedy: valid call, attachment untouched=True', 0, 'greedy: unknown stop rule'),
    ('gitcap_greedy: not finalized', -2, 'weights not finalized'),
    ('gitcap_greedy: not finalized, stop 7', -1, 'greedy: unknown stop rule'),
    ('gitcap_greedy_raw: not finalized', -2, 'weights not finalized'),
    ('gitcap_greedy_raw: not finalized, stop 7', -1, 'greedy: unknown stop rule'),
    ('gitcap_greedy_submit: not finalized', -2, 'weights not finalized'),
    ('gitcap_greedy_submit: not finalized, stop 7', -1, 'greedy: unknown stop rule'),
    ('gitcap_greedy_raw_submit: not finalized', -2, 'weights not finalized'),
    ('gitcap_greedy_raw_submit: not finalized, stop 7', -1, 'greedy: unknown stop rule'),
    ('gitcap_beam_search: not finalized', -2, 'weights not finalized'),
    ('gitcap_beam_search_submit: not finalized', -2, 'weights not finalized'),
    ('gitcap_beam_search_raw_submit: not finalized', -2, 'weights not finalized'),
    ('gitcap_window_greedy: not finalized', -2, 'window: fewer than F frames pushed since the reset'),
    ('gitcap_window_beam_search: not finalized', -2, 'window: fewer than F frames pushed since the reset'),
]

STUDENT_EXPECTED = [
    ('gitcap_student_greedy: null handle', -1, 'student_greedy: null handle'),
    ('gitcap_student_greedy [no window]: null ids_out', -1, 'student_greedy: bad arguments'),
    ('gitcap_student_greedy [no window]: max_len 0', -1, 'student_greedy: bad arguments'),
    ('gitcap_student_greedy [no window]: max_len 9', -1, 'student_greedy: max_len exceeds max_text_len'),
    ('gitcap_student_greedy [no window]: stop 7', -1, 'student_greedy: unknown stop rule'),
    ('gitcap_student_greedy [no window]: attached ld 5', -1,
     'student_greedy: the attached token log-probability buffer has ld < max_len'),
    ('gitcap_student_greedy [no window]: attached ld 5 and stop 7', -1, 'student_greedy: unknown stop rule'),
    ('gitcap_student_greedy [no window]: null memory', -1, 'student: set_memory: bad arguments / B exceeds max_rows'),
    ('gitcap_student_greedy [no window]: B 0', -1, 'student: set_memory: bad arguments / B exceeds max_rows'),
    ('gitcap_student_greedy [no window]: B 3', -1, 'student: set_memory: bad arguments / B exceeds max_rows'),
    ('gitcap_student_window_greedy: null handle', -1, 'student_window_greedy: null handle'),
    ('gitcap_student_window_greedy [no window]: null ids_out', -1, 'student_window_greedy: bad arguments'),
    ('gitcap_student_window_greedy [no window]: max_len 0', -1, 'student_window_greedy: bad arguments'),
    ('gitcap_student_window_greedy [no window]: max_len 9', -1, 'student_window_greedy: max_len exceeds max_text_len'),
    ('gitcap_student_window_greedy [no window]: stop 7', -1, 'student_window_greedy: unknown stop rule'),
    ('gitcap_student_window_greedy [no window]: attached ld 5', -1,
     'student_window_greedy: the attached token log-probability buffer has ld < max_len'),
    ('gitcap_student_window_greedy [no window]: attached ld 5 and stop 7', -1, 'student_window_greedy: unknown stop rule'),
    ('gitcap_student_window_greedy: no window', -2, 'student_window_greedy: fewer than mem_tokens tokens pushed since the reset'),
    ('gitcap_student_greedy_draft: null handle', -1, 'student_greedy_draft: null handle'),
    ('gitcap_student_greedy_draft [no window]: null ids_out', -1, 'student_greedy_draft: bad arguments'),
    ('gitcap_student_greedy_draft [no window]: max_len 0', -1, 'student_greedy_draft: bad arguments'),
    ('gitcap_student_greedy_draft [no window]: max_len 9', -1, 'student_greedy_draft: max_len exceeds max_text_len'),
    ('gitcap_student_greedy_draft [no window]: stop 7', -1, 'student_greedy_draft: unknown stop rule'),
    ('gitcap_student_greedy_draft [no window]: attached ld 5', -1,
     'student_greedy_draft: the attached token log-probability buffer has ld < max_len'),
    ('gitcap_student_greedy_draft [no window]: attached ld 5 and stop 7', -1, 'student_greedy_draft: unknown stop rule'),
    ('gitcap_student_greedy_draft [no window]: null draft_ids', -1, 'student_greedy_draft: null draft_ids'),
    ('gitcap_student_greedy_draft [no window]: n_draft 0', -1,
     'student_greedy_draft: n_draft outside [1, max_len], or ld_draft < n_draft + 1'),
    ('gitcap_student_greedy_draft [no window]: n_draft 7', -1,
     'student_greedy_draft: n_draft outside [1, max_len], or ld_draft < n_draft + 1'),
    ('gitcap_student_greedy_draft [no window]: ld_draft 6', -1,
     'student_greedy_draft: n_draft outside [1, max_len], or ld_draft < n_draft + 1'),
    ('gitcap_student_greedy_draft [no window]: attached ld 5 and null draft_ids', -1,
     'student_greedy_draft: the attached token log-probability buffer has ld < max_len'),
    ('gitcap_student_greedy_draft [no window]: null memory', -1, 'student: set_memory: bad arguments / B exceeds max_rows'),
    ('gitcap_student_greedy_draft [no window]: B 0', -1, 'student: set_memory: bad arguments / B exceeds max_rows'),
    ('gitcap_student_greedy_draft [no window]: B 3', -1, 'student: set_memory: bad arguments / B exceeds max_rows'),
    ('gitcap_student_window_greedy_draft: null handle', -1, 'student_window_greedy_draft: null handle'),
    ('gitcap_student_window_greedy_draft [no window]: null ids_out', -1, 'student_window_greedy_draft: bad arguments'),
    ('gitcap_student_window_greedy_draft [no window]: max_len 0', -1, 'student_window_greedy_draft: bad arguments'),
    ('gitcap_student_window_greedy_draft [no window]: max_len 9', -1, 'student_window_greedy_draft: max_len exceeds max_text_len'),
    ('gitcap_student_window_greedy_draft [no window]: stop 7', -1, 'student_window_greedy_draft: unknown stop rule'),
    ('gitcap_student_window_greedy_draft [no window]: attached ld 5', -1,
     'student_window_greedy_draft: the attached token log-probability buffer has ld < max_len'),
    ('gitcap_student_window_greedy_draft [no window]: attached ld 5 and stop 7', -1,
     'student_window_greedy_draft: unknown stop rule'),
    ('gitcap_student_window_greedy_draft [no window]: null draft_ids', -1, 'student_window_greedy_draft: null draft_ids'),
    ('gitcap_student_window_greedy_draft [no window]: n_draft 0', -1,
     'student_window_greedy_draft: n_draft outside [1, max_len], or ld_draft < n_draft + 1'),
    ('gitcap_student_window_greedy_draft [no window]: n_draft 7', -1,
     'student_window_greedy_draft: n_draft outside [1, max_len], or ld_draft < n_draft + 1'),
    ('gitcap_student_window_greedy_draft [no window]: ld_draft 6', -1,
     'student_window_greedy_draft: n_draft outside [1, max_len], or ld_draft < n_draft + 1'),
    ('gitcap_student_window_greedy_draft [no window]: attached ld 5 and null draft_ids', -1,
     'student_window_greedy_draft: the attached token log-probability buffer has ld < max_len'),
    ('gitcap_student_window_greedy_draft: no window', -2,
     'student_window_greedy_draft: fewer than mem_tokens tokens pushed since the reset'),
    ('gitcap_student_window_greedy: empty window', -2,
     'student_window_greedy: fewer than mem_tokens tokens pushed since the reset'),
    ('gitcap_student_window_greedy_draft: empty window', -2,
     'student_window_greedy_draft: fewer than mem_tokens tokens pushed since the reset'),
    ('gitcap_student_window_greedy: F - 1 tokens', -2,
     'student_window_greedy: fewer than mem_tokens tokens pushed since the reset'),
    ('gitcap_student_window_greedy: F - 1 tokens, stop 7', -1, 'student_window_greedy: unknown stop rule'),
    ('gitcap_student_window_greedy_draft: F - 1 tokens', -2,
     'student_window_greedy_draft: fewer than mem_tokens tokens pushed since the reset'),
    ('gitcap_student_window_greedy_draft: F - 1 tokens, stop 7', -1, 'student_window_greedy_draft: unknown stop rule'),
    ('gitcap_student_window_greedy_draft: F - 1 tokens, n_draft 0', -1,
     'student_window_greedy_draft: n_draft outside [1, max_len], or ld_draft < n_draft + 1'),
    ('gitcap_student_greedy: attached, null ids_out', -1, 'student_greedy: bad arguments'),
    ('gitcap_student_greedy: valid call, attachment untouched=True', 0, 'student_greedy: bad arguments'),
    ('gitcap_student_window_greedy [full window]: null ids_out', -1, 'student_window_greedy: bad arguments'),
    ('gitcap_student_window_greedy [full window]: max_len 0', -1, 'student_window_greedy: bad arguments'),
    ('gitcap_student_window_greedy [full window]: max_len 9', -1, 'student_window_greedy: max_len exceeds max_text_len'),
    ('gitcap_student_window_greedy [full window]: stop 7', -1, 'student_window_greedy: unknown stop rule'),
    ('gitcap_student_window_greedy [full window]: attached ld 5', -1,
     'student_window_greedy: the attached token log-probability buffer has ld < max_len'),
    ('gitcap_student_window_greedy [full window]: attached ld 5 and stop 7', -1, 'student_window_greedy: unknown stop rule'),
    ('gitcap_student_window_greedy: attached, null ids_out', -1, 'student_window_greedy: bad arguments'),
    ('gitcap_student_window_greedy: valid call, attachment untouched=True', 0, 'student_window_greedy: bad arguments'),
    ('gitcap_student_greedy_draft: attached, null ids_out', -1, 'student_greedy_draft: bad arguments'),
    ('gitcap_student_greedy_draft: valid call, attachment untouched=True', 0, 'student_greedy_draft: bad arguments'),
    ('gitcap_student_window_greedy_draft [full window]: null ids_out', -1, 'student_window_greedy_draft: bad arguments'),
    ('gitcap_student_window_greedy_draft [full window]: max_len 0', -1, 'student_window_greedy_draft: bad arguments'),
    ('gitcap_student_window_greedy_draft [full window]: max_len 9', -1,
     'student_window_greedy_draft: max_len exceeds max_text_len'),
    ('gitcap_student_window_greedy_draft [full window]: stop 7', -1, 'student_window_greedy_draft: unknown stop rule'),
    ('gitcap_student_window_greedy_draft [full window]: attached ld 5', -1,
     'student_window_greedy_draft: the attached token log-probability buffer has ld < max_len'),
    ('gitcap_student_window_greedy_draft [full window]: attached ld 5 and stop 7', -1,
     'student_window_greedy_draft: unknown stop rule'),
    ('gitcap_student_window_greedy_draft [full window]: null draft_ids', -1, 'student_window_greedy_draft: null draft_ids'),
    ('gitcap_student_window_greedy_draft [full window]: n_draft 0', -1,
     'student_window_greedy_draft: n_draft outside [1, max_len], or ld_draft < n_draft + 1'),
    ('gitcap_student_window_greedy_draft [full window]: n_draft 7', -1,
     'student_window_greedy_draft: n_draft outside [1, max_len], or ld_draft < n_draft + 1'),
    ('gitcap_student_window_greedy_draft [full window]: ld_draft 6', -1,
     'student_window_greedy_draft: n_draft outside [1, max_len], or ld_draft < n_draft + 1'),
    ('gitcap_student_window_greedy_draft [full window]: attached ld 5 and null draft_ids', -1,
     'student_window_greedy_draft: the attached token log-probability buffer has ld < max_len'),
    ('gitcap_student_window_greedy_draft: attached, null ids_out', -1, 'student_window_greedy_draft: bad arguments'),
    ('gitcap_student_window_greedy_draft: valid call, attachment untouched=True', 0, 'student_window_greedy_draft: bad arguments'),
    ('gitcap_student_attach_token_logprobs: not finalized', -2, 'student_attach_token_logprobs: weights not finalized'),
    ('gitcap_student_greedy: not finalized', -2, 'student: weights not finalized'),
    ('gitcap_student_greedy: not finalized, stop 7', -1, 'student_greedy: unknown stop rule'),
    ('gitcap_student_window_greedy: not finalized', -2, 'student_window_greedy: weights not finalized'),
    ('gitcap_student_window_greedy: not finalized, stop 7', -1, 'student_window_greedy: unknown stop rule'),
    ('gitcap_student_greedy_draft: not finalized', -2, 'student: weights not finalized'),
    ('gitcap_student_greedy_draft: not finalized, stop 7', -1, 'student_greedy_draft: unknown stop rule'),
    ('gitcap_student_window_greedy_draft: not finalized', -2, 'student_window_greedy_draft: weights not finalized'),
    ('gitcap_student_window_greedy_draft: not finalized, stop 7', -1, 'student_window_greedy_draft: unknown stop rule'),
    ('gitcap_student_window_greedy: not finalized, empty window', -2, 'student_window_greedy: weights not finalized'),
    ('gitcap_student_window_greedy_draft: not finalized, empty window', -2, 'student_window_greedy_draft: weights not finalized'),
]


def _compare(got, want):
    for g, w in zip(got, want):
        assert g == w, (g, w)
    assert len(got) == len(want) and len(want) > 50, (len(got), len(want))


def test_teacher_entry_point_errors():
    _compare(_teacher_observed(), TEACHER_EXPECTED)


def test_student_entry_point_errors():
    _compare(_student_observed(), STUDENT_EXPECTED)
