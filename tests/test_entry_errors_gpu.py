"""Status code and exact *_last_error text of every argument check and state check of the greedy and beam entry points of the
teacher (gitcap_greedy, _raw, _submit, _raw_submit, gitcap_beam_search, _submit, _raw_submit, gitcap_window_greedy,
gitcap_window_beam_search) and of the student (gitcap_student_greedy, _window_greedy, _greedy_draft, _window_greedy_draft), on
git_tiny(2) and the tiny student.

The entry points of a family run one shared body; what differs between them (the synchronous raw path does not run the raw-frame
checks the submitted one runs, the window forms check the window behind the arguments) is pinned here as recorded behaviour.  The
tables were recorded on the commit before the entry points were folded.  No arithmetic: a refused call launches nothing.  The
"sizes overflow" case is driven through the submitted raw paths only: the synchronous raw path has no such check and would launch.

An attachment (gitcap_attach_token_logprobs and its student twin) is consumed by a call that then fails its argument check.

STUDENT_MORE_EXPECTED does the same for gitcap_student_pool_greedy, gitcap_student_beam_search and
gitcap_student_window_beam_search, and adds, for every student entry point, which of the five one-shot attachments (token
log-probabilities, top-k, constraints, prompt, frame counts) are still pending behind a valid and behind a refused call: seen()."""
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


# ---- student: the pool call, the two beam searches, and what every entry point leaves pending ------------------------------------

MORE = ("gitcap_student_pool_greedy", "gitcap_student_beam_search", "gitcap_student_window_beam_search")
TOK, BAN = 5, 80        # the attached prompt is [CLS, TOK] for both clips; the attached constraints suppress the ids 0 .. BAN - 1


class _StudentMore(_Student):
    def __init__(self, weights=True):
        super().__init__(weights)
        F, V = self.cfg.mem_tokens, self.cfg.vocab_length
        self.sid = (ctypes.c_int32 * 2)(0, 1)
        self.frames = (ctypes.c_int32 * 2)()
        self.counts = (ctypes.c_int32 * 2)(F, F)
        self.tki = torch.full((2, S_LEN, 2), -1, dtype=torch.int64, device="cuda")
        self.tkl = torch.full((2, S_LEN, 2), POISON, device="cuda")
        self.sup = torch.arange(V - 2, dtype=torch.int32, device="cuda")
        self.prm = torch.tensor([[self.cfg.cls_token_id] + [TOK] * L] * 2, dtype=torch.int64, device="cuda")
        self.plen = torch.full((2,), 2, dtype=torch.int32, device="cuda")
        self.bout = torch.full((2, L + 2), -1, dtype=torch.int64, device="cuda")
        self.logits = torch.zeros((2, S_LEN, V), device="cuda")
        self.mass = torch.zeros((2 * S_LEN, F), device="cuda")
        self.pool_tokens = self.mem.reshape(2 * F, -1).contiguous()
        self.pool_ids = (ctypes.c_int32 * (2 * F))(*([0] * F + [1] * F))

    def more(self, name, h=True, sid="own", mem="own", B=2, k=1, max_len=S_LEN, stop=0, ids="own"):
        hh = self.h if h else None
        if name == MORE[0]:
            return self.lib.gitcap_student_pool_greedy(hh, self.sid if sid == "own" else sid, B, max_len, stop,
                                                       _p(self.ids) if ids == "own" else ids, _p(self.steps), self.frames, stream())
        out = _p(self.bout) if ids == "own" else ids
        if name == MORE[1]:
            return self.lib.gitcap_student_beam_search(hh, _p(self.mem) if mem == "own" else mem, B, k, max_len, out, stream())
        return self.lib.gitcap_student_window_beam_search(hh, k, max_len, out, stream())

    def attach_tk(self, ld=S_LEN):
        assert self.lib.gitcap_student_attach_top_logprobs(self.h, 2, _p(self.tki), _p(self.tkl), ld) == 0

    def attach_co(self, n=BAN):
        from gitcap._lib import CConstraints
        c = CConstraints(0, 0, self.sup.data_ptr(), n)
        assert self.lib.gitcap_student_attach_constraints(self.h, ctypes.byref(c)) == 0

    def attach_pr(self, max_len=2):
        assert self.lib.gitcap_student_attach_prompt(self.h, _p(self.prm), L + 1, _p(self.plen), 2, max_len) == 0

    def attach_fc(self, B=2):
        assert self.lib.gitcap_student_attach_frame_counts(self.h, self.counts, B) == 0

    def fill_window(self):
        assert self.lib.gitcap_student_window_reset(self.h, 2) == 0
        assert self.lib.gitcap_student_window_push(self.h, _p(self.mem), 2, self.cfg.mem_tokens, stream()) == 0

    def fill_pool(self):
        assert self.lib.gitcap_student_pool_reset(self.h, 2) == 0
        assert self.lib.gitcap_student_pool_push(self.h, _p(self.pool_tokens), self.pool_ids, 2 * self.cfg.mem_tokens, stream()) == 0

    def seen(self):
        """Which attachments are still pending: the counts by the message of a window push that is refused either way (it refuses and
        clears them, and takes nothing else), the other four by what the gitcap_student_greedy behind it does with them."""
        self.lib.gitcap_student_window_push(self.h, None, 2, 1, stream())
        fc = b"frame counts are attached" in self.lib.gitcap_student_last_error(self.h)
        self.lp.fill_(POISON)
        self.tkl.fill_(POISON)
        self.ids.fill_(-1)
        rc = self.call("gitcap_student_greedy")
        torch.cuda.synchronize()
        return "greedy=%d fc=%d lp=%d tk=%d co=%d pr=%d" % (rc, fc, bool((self.lp != POISON).any()), bool((self.tkl != POISON).any()),
                                                             bool((self.ids[:, 2:] >= BAN).all()), bool((self.ids[:, 1] == TOK).all()))

    def pending(self, label, valid, bad, restore=None):
        for what, fn, fc in (("all five, valid arguments", valid, True), ("all five, a bad argument", bad, True),
                             ("all but the counts, valid arguments", valid, False)):
            self.attach(S_LEN)
            self.attach_tk()
            self.attach_co()
            self.attach_pr()
            if fc:
                self.attach_fc()
            self.rec(f"{label}: {what}", fn())
            torch.cuda.synchronize()
            self.rows.append((f"{label}: {what}, then", 0, self.seen()))
            if restore:
                restore()


def _student_more_observed():
    t = _StudentMore()
    pool, beam, wbeam = MORE
    for name in MORE:
        t.rec(f"{name}: null handle", t.more(name, h=False), h=False)
    t.rec(f"{pool}: no pool", t.more(pool))
    t.rec(f"{pool}: no pool, max_len 0", t.more(pool, max_len=0))
    t.rec(f"{pool}: no pool, B 0", t.more(pool, B=0))
    t.rec(f"{wbeam}: no window", t.more(wbeam))
    t.rec(f"{wbeam}: no window, k 0", t.more(wbeam, k=0))
    assert t.lib.gitcap_student_window_reset(t.h, 2) == 0
    t.rec(f"{wbeam}: empty window", t.more(wbeam))
    assert t.lib.gitcap_student_pool_reset(t.h, 2) == 0
    t.rec(f"{pool}: empty streams", t.more(pool))
    t.rec(f"{pool}: empty streams, stream 5", t.more(pool, sid=(ctypes.c_int32 * 2)(0, 5)))
    t.fill_window()
    t.fill_pool()
    assert t.lib.gitcap_student_pool_drop(t.h, 1) == 0
    t.rec(f"{pool}: stream 1 empty", t.more(pool))
    t.rec(f"{pool}: stream 1 empty, named twice", t.more(pool, sid=(ctypes.c_int32 * 2)(1, 1)))
    t.fill_pool()
    for name in MORE:
        c = lambda **kw: t.more(name, **kw)                                         # noqa: E731
        t.rec(f"{name}: null ids_out", c(ids=None))
        t.rec(f"{name}: max_len 0", c(max_len=0))
        t.rec(f"{name}: max_len 1", c(max_len=1))
        t.rec(f"{name}: max_len 9", c(max_len=L + 1))
        t.rec(f"{name}: max_len 10", c(max_len=L + 2))
        if name == pool:
            t.rec(f"{name}: stop 7", c(stop=7))
            t.rec(f"{name}: null stream_ids", c(sid=None))
            t.rec(f"{name}: null stream_ids, max_len 0", c(sid=None, max_len=0))
            t.rec(f"{name}: stream 2", c(sid=(ctypes.c_int32 * 2)(0, 2)))
            t.rec(f"{name}: stream -1", c(sid=(ctypes.c_int32 * 2)(-1, 1)))
            t.rec(f"{name}: stream 0 twice", c(sid=(ctypes.c_int32 * 2)(0, 0)))
            t.rec(f"{name}: B 0, stop 7", c(B=0, stop=7))
            t.attach(S_LEN - 1)
            t.rec(f"{name}: attached ld 5", c())
            t.attach(S_LEN - 1)
            t.rec(f"{name}: attached ld 5 and stop 7", c(stop=7))
            t.attach(S_LEN - 1)
            t.rec(f"{name}: attached ld 5 and B 0", c(B=0))
            t.attach(S_LEN - 1)
            t.rec(f"{name}: attached ld 5 and null stream_ids", c(sid=None))
            t.attach_tk(S_LEN - 1)
            t.rec(f"{name}: attached top-k ld 5", c())
            t.attach_tk(S_LEN - 1)
            t.rec(f"{name}: attached top-k ld 5 and stream 2", c(sid=(ctypes.c_int32 * 2)(0, 2)))
        else:
            t.rec(f"{name}: k 0", c(k=0))
            t.rec(f"{name}: k 17", c(k=17))
            t.rec(f"{name}: k 2", c(k=2))
            t.rec(f"{name}: k 17, max_len 10", c(k=17, max_len=L + 2))
            # a log-probability buffer with a short ld is not this call's: it stays for the greedy call behind it
            t.attach(S_LEN - 1)
            t.rec(f"{name}: attached ld 5", c())
            t.rec(f"{name}: attached ld 5, then k 0", c(k=0))
            t.rec(f"{name}: attached ld 5, then gitcap_student_greedy", t.call("gitcap_student_greedy"))
        if name != wbeam:
            t.rec(f"{name}: B 0", c(B=0))
            t.rec(f"{name}: B 3", c(B=3))
        if name == beam:
            t.rec(f"{name}: null memory", c(mem=None))
            t.rec(f"{name}: null memory, k 0", c(mem=None, k=0))
            t.attach_fc(1)
            t.rec(f"{name}: attached counts of 1 clip", c())
            t.attach_fc(1)
            t.rec(f"{name}: attached counts of 1 clip and k 0", c(k=0))
        else:
            t.attach_fc()
            t.rec(f"{name}: attached counts", c())
            t.attach_fc()
            t.rec(f"{name}: attached counts and max_len 0", c(max_len=0))
        t.attach_co(t.cfg.vocab_length - 2)
        t.rec(f"{name}: attached constraints ban every column", c())
        t.attach_co(t.cfg.vocab_length - 2)
        t.rec(f"{name}: attached constraints ban every column and max_len 10", c(max_len=L + 2))
        t.attach_pr(S_LEN + 1)
        t.rec(f"{name}: attached prompt of 7", c())
        t.attach_pr(S_LEN + 1)
        t.attach_co(t.cfg.vocab_length - 2)
        t.rec(f"{name}: attached prompt of 7 and constraints ban every column", c())
        rc = c()
        torch.cuda.synchronize()
        t.rec(f"{name}: valid call", rc)
    t.rec(f"{beam}: 1 clip x 2 beams", t.more(beam, B=1, k=2))
    torch.cuda.synchronize()

    # what stays pending: one block per entry point, the attachments set before it and seen() behind it
    lib, h, F, part = t.lib, t.h, t.cfg.mem_tokens, t.mem[:, :1].contiguous()
    one = (ctypes.c_int32 * 1)(0)
    cnt = (ctypes.c_int32 * 2)()
    for name in STUDENT:
        t.pending(name, lambda: t.call(name), lambda: t.call(name, max_len=0))
    t.pending("gitcap_student_window_greedy_partial",
              lambda: lib.gitcap_student_window_greedy_partial(h, S_LEN, 0, _p(t.ids), _p(t.steps), t.frames, stream()),
              lambda: lib.gitcap_student_window_greedy_partial(h, 0, 0, _p(t.ids), _p(t.steps), t.frames, stream()))
    t.pending(pool, lambda: t.more(pool), lambda: t.more(pool, max_len=0))
    t.pending(beam, lambda: t.more(beam), lambda: t.more(beam, k=0))
    t.pending(wbeam, lambda: t.more(wbeam), lambda: t.more(wbeam, k=0))
    score = lambda T: lib.gitcap_student_score(h, _p(t.d), S_LEN + 1, 2, T, None, -1, None, 0, None, None, None, None, stream())   # noqa: E731
    t.pending("gitcap_student_score", lambda: score(S_LEN + 1), lambda: score(1))
    t.pending("gitcap_student_set_memory", lambda: lib.gitcap_student_set_memory(h, _p(t.mem), 2, stream()),
              lambda: lib.gitcap_student_set_memory(h, _p(t.mem), 0, stream()))
    t.pending("gitcap_student_window_reset", lambda: lib.gitcap_student_window_reset(h, 2), lambda: lib.gitcap_student_window_reset(h, -1),
              restore=t.fill_window)
    t.pending("gitcap_student_window_push", lambda: lib.gitcap_student_window_push(h, _p(part), 2, 1, stream()),
              lambda: lib.gitcap_student_window_push(h, _p(part), 2, F + 1, stream()))
    t.pending("gitcap_student_pool_reset", lambda: lib.gitcap_student_pool_reset(h, 2), lambda: lib.gitcap_student_pool_reset(h, -1),
              restore=t.fill_pool)
    t.pending("gitcap_student_pool_push", lambda: lib.gitcap_student_pool_push(h, _p(part), one, 1, stream()),
              lambda: lib.gitcap_student_pool_push(h, _p(part), one, 0, stream()))
    t.pending("gitcap_student_pool_drop", lambda: lib.gitcap_student_pool_drop(h, 0), lambda: lib.gitcap_student_pool_drop(h, 7), restore=t.fill_pool)
    t.pending("gitcap_student_pool_counts", lambda: lib.gitcap_student_pool_counts(h, cnt), lambda: lib.gitcap_student_pool_counts(h, None))
    att = lambda T: lib.gitcap_student_attention(h, _p(t.d), S_LEN + 1, 2, T, -1, None, _p(t.mass), F, stream())                    # noqa: E731
    t.pending("gitcap_student_attention", lambda: att(S_LEN), lambda: att(0))
    fwd = lambda out: lib.gitcap_student_forward_decoder(h, _p(t.d), S_LEN + 1, 2, S_LEN, out, stream())                             # noqa: E731
    t.pending("gitcap_student_forward_decoder", lambda: fwd(_p(t.logits)), lambda: fwd(None))

    # before gitcap_student_finalize
    u = _StudentMore(weights=False)
    for name in MORE:
        u.rec(f"{name}: not finalized", u.more(name))
        u.rec(f"{name}: not finalized, max_len 0", u.more(name, max_len=0))
    u.rec(f"{pool}: not finalized, B 0", u.more(pool, B=0))
    u.rec(f"{pool}: not finalized, stop 7", u.more(pool, stop=7))
    u.rec(f"{beam}: not finalized, k 0", u.more(beam, k=0))
    u.rec(f"{wbeam}: not finalized, k 0", u.more(wbeam, k=0))
    assert u.lib.gitcap_student_window_reset(u.h, 2) == 0
    u.rec(f"{wbeam}: not finalized, empty window", u.more(wbeam))
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

# recorded on the commit before the student got one pending record and one greedy / beam entry (see _student_more_observed)
STUDENT_MORE_EXPECTED = [('gitcap_student_pool_greedy: null handle', -1, 'student_pool_greedy: null handle'),
 ('gitcap_student_beam_search: null handle', -1, 'student_beam_search: null handle'),
 ('gitcap_student_window_beam_search: null handle', -1, 'student_window_beam_search: null handle'),
 ('gitcap_student_pool_greedy: no pool', -2, 'student_pool_greedy: no pool (gitcap_student_pool_reset first)'),
 ('gitcap_student_pool_greedy: no pool, max_len 0', -1, 'student_pool_greedy: bad arguments'),
 ('gitcap_student_pool_greedy: no pool, B 0', -1, 'student_pool_greedy: B outside [1, max_rows]'),
 ('gitcap_student_window_beam_search: no window', -2, 'student_window_beam_search: no window (gitcap_student_window_reset first)'),
 ('gitcap_student_window_beam_search: no window, k 0', -2, 'student_window_beam_search: no window (gitcap_student_window_reset first)'),
 ('gitcap_student_window_beam_search: empty window', -2, 'student_window_beam_search: fewer than mem_tokens tokens pushed since the reset'),
 ('gitcap_student_pool_greedy: empty streams', -2, 'student_pool_greedy: stream 0 holds no token'),
 ('gitcap_student_pool_greedy: empty streams, stream 5', -1, 'student_pool_greedy: row 1 names stream 5, outside [0, 2)'),
 ('gitcap_student_pool_greedy: stream 1 empty', -2, 'student_pool_greedy: stream 1 holds no token'),
 ('gitcap_student_pool_greedy: stream 1 empty, named twice', -1, 'student_pool_greedy: stream 1 is named twice'),
 ('gitcap_student_pool_greedy: null ids_out', -1, 'student_pool_greedy: bad arguments'),
 ('gitcap_student_pool_greedy: max_len 0', -1, 'student_pool_greedy: bad arguments'),
 ('gitcap_student_pool_greedy: max_len 1', 0, 'student_pool_greedy: bad arguments'),
 ('gitcap_student_pool_greedy: max_len 9', -1, 'student_pool_greedy: max_len exceeds max_text_len'),
 ('gitcap_student_pool_greedy: max_len 10', -1, 'student_pool_greedy: max_len exceeds max_text_len'),
 ('gitcap_student_pool_greedy: stop 7', -1, 'student_pool_greedy: unknown stop rule'),
 ('gitcap_student_pool_greedy: null stream_ids', -1, 'student_pool_greedy: bad arguments'),
 ('gitcap_student_pool_greedy: null stream_ids, max_len 0', -1, 'student_pool_greedy: bad arguments'),
 ('gitcap_student_pool_greedy: stream 2', -1, 'student_pool_greedy: row 1 names stream 2, outside [0, 2)'),
 ('gitcap_student_pool_greedy: stream -1', -1, 'student_pool_greedy: row 0 names stream -1, outside [0, 2)'),
 ('gitcap_student_pool_greedy: stream 0 twice', -1, 'student_pool_greedy: stream 0 is named twice'),
 ('gitcap_student_pool_greedy: B 0, stop 7', -1, 'student_pool_greedy: unknown stop rule'),
 ('gitcap_student_pool_greedy: attached ld 5', -1, 'student_pool_greedy: the attached token log-probability buffer has ld < max_len'),
 ('gitcap_student_pool_greedy: attached ld 5 and stop 7', -1, 'student_pool_greedy: unknown stop rule'),
 ('gitcap_student_pool_greedy: attached ld 5 and B 0',
  -1,
  'student_pool_greedy: the attached token log-probability buffer has ld < max_len'),
 ('gitcap_student_pool_greedy: attached ld 5 and null stream_ids', -1, 'student_pool_greedy: bad arguments'),
 ('gitcap_student_pool_greedy: attached top-k ld 5',
  -1,
  'student_pool_greedy: the attached top-k buffers have ld < the positions the call writes'),
 ('gitcap_student_pool_greedy: attached top-k ld 5 and stream 2',
  -1,
  'student_pool_greedy: the attached top-k buffers have ld < the positions the call writes'),
 ('gitcap_student_pool_greedy: B 0', -1, 'student_pool_greedy: B outside [1, max_rows]'),
 ('gitcap_student_pool_greedy: B 3', -1, 'student_pool_greedy: B outside [1, max_rows]'),
 ('gitcap_student_pool_greedy: attached counts',
  -1,
  'student_pool_greedy: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_pool_greedy: attached counts and max_len 0',
  -1,
  'student_pool_greedy: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_pool_greedy: attached constraints ban every column',
  -1,
  'student_pool_greedy: the attached constraints could ban every column of a row (n_suppress + max_len >= vocab_size)'),
 ('gitcap_student_pool_greedy: attached constraints ban every column and max_len 10',
  -1,
  'student_pool_greedy: max_len exceeds max_text_len'),
 ('gitcap_student_pool_greedy: attached prompt of 7', -1, 'student_pool_greedy: the attached prompt is longer than max_len'),
 ('gitcap_student_pool_greedy: attached prompt of 7 and constraints ban every column',
  -1,
  'student_pool_greedy: the attached constraints could ban every column of a row (n_suppress + max_len >= vocab_size)'),
 ('gitcap_student_pool_greedy: valid call',
  0,
  'student_pool_greedy: the attached constraints could ban every column of a row (n_suppress + max_len >= vocab_size)'),
 ('gitcap_student_beam_search: null ids_out', -1, 'student_beam_search: bad arguments'),
 ('gitcap_student_beam_search: max_len 0', -1, 'student_beam_search: bad arguments'),
 ('gitcap_student_beam_search: max_len 1', -1, 'student_beam_search: bad arguments'),
 ('gitcap_student_beam_search: max_len 9', 0, 'student_beam_search: bad arguments'),
 ('gitcap_student_beam_search: max_len 10', -1, 'student_beam_search: max_len exceeds max_text_len + 1'),
 ('gitcap_student_beam_search: k 0', -1, 'student_beam_search: bad arguments'),
 ('gitcap_student_beam_search: k 17', -1, 'student_beam_search: at most 16 beams'),
 ('gitcap_student_beam_search: k 2', -1, 'student_beam_search: B * k exceeds max_rows'),
 ('gitcap_student_beam_search: k 17, max_len 10', -1, 'student_beam_search: at most 16 beams'),
 ('gitcap_student_beam_search: attached ld 5', 0, 'student_beam_search: at most 16 beams'),
 ('gitcap_student_beam_search: attached ld 5, then k 0', -1, 'student_beam_search: bad arguments'),
 ('gitcap_student_beam_search: attached ld 5, then gitcap_student_greedy',
  -1,
  'student_greedy: the attached token log-probability buffer has ld < max_len'),
 ('gitcap_student_beam_search: B 0', -1, 'student_beam_search: bad arguments'),
 ('gitcap_student_beam_search: B 3', -1, 'student_beam_search: B * k exceeds max_rows'),
 ('gitcap_student_beam_search: null memory', -1, 'student_beam_search: bad arguments'),
 ('gitcap_student_beam_search: null memory, k 0', -1, 'student_beam_search: bad arguments'),
 ('gitcap_student_beam_search: attached counts of 1 clip', -1, 'student_beam_search: B = 2, but frame counts of 1 clips are attached'),
 ('gitcap_student_beam_search: attached counts of 1 clip and k 0', -1, 'student_beam_search: bad arguments'),
 ('gitcap_student_beam_search: attached constraints ban every column',
  -1,
  'student_beam_search: the attached constraints could ban every column of a row (n_suppress + max_len >= vocab_size)'),
 ('gitcap_student_beam_search: attached constraints ban every column and max_len 10',
  -1,
  'student_beam_search: max_len exceeds max_text_len + 1'),
 ('gitcap_student_beam_search: attached prompt of 7', -1, 'student_beam_search: the attached prompt is longer than max_len - 1'),
 ('gitcap_student_beam_search: attached prompt of 7 and constraints ban every column',
  -1,
  'student_beam_search: the attached constraints could ban every column of a row (n_suppress + max_len >= vocab_size)'),
 ('gitcap_student_beam_search: valid call',
  0,
  'student_beam_search: the attached constraints could ban every column of a row (n_suppress + max_len >= vocab_size)'),
 ('gitcap_student_window_beam_search: null ids_out', -1, 'student_window_beam_search: bad arguments'),
 ('gitcap_student_window_beam_search: max_len 0', -1, 'student_window_beam_search: bad arguments'),
 ('gitcap_student_window_beam_search: max_len 1', -1, 'student_window_beam_search: bad arguments'),
 ('gitcap_student_window_beam_search: max_len 9', 0, 'student_window_beam_search: bad arguments'),
 ('gitcap_student_window_beam_search: max_len 10', -1, 'student_window_beam_search: max_len exceeds max_text_len + 1'),
 ('gitcap_student_window_beam_search: k 0', -1, 'student_window_beam_search: bad arguments'),
 ('gitcap_student_window_beam_search: k 17', -1, 'student_window_beam_search: at most 16 beams'),
 ('gitcap_student_window_beam_search: k 2', -1, 'student_window_beam_search: B * k exceeds max_rows'),
 ('gitcap_student_window_beam_search: k 17, max_len 10', -1, 'student_window_beam_search: at most 16 beams'),
 ('gitcap_student_window_beam_search: attached ld 5', 0, 'student_window_beam_search: at most 16 beams'),
 ('gitcap_student_window_beam_search: attached ld 5, then k 0', -1, 'student_window_beam_search: bad arguments'),
 ('gitcap_student_window_beam_search: attached ld 5, then gitcap_student_greedy',
  -1,
  'student_greedy: the attached token log-probability buffer has ld < max_len'),
 ('gitcap_student_window_beam_search: attached counts',
  -1,
  'student_window_beam_search: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_window_beam_search: attached counts and max_len 0',
  -1,
  'student_window_beam_search: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_window_beam_search: attached constraints ban every column',
  -1,
  'student_window_beam_search: the attached constraints could ban every column of a row (n_suppress + max_len >= vocab_size)'),
 ('gitcap_student_window_beam_search: attached constraints ban every column and max_len 10',
  -1,
  'student_window_beam_search: max_len exceeds max_text_len + 1'),
 ('gitcap_student_window_beam_search: attached prompt of 7',
  -1,
  'student_window_beam_search: the attached prompt is longer than max_len - 1'),
 ('gitcap_student_window_beam_search: attached prompt of 7 and constraints ban every column',
  -1,
  'student_window_beam_search: the attached constraints could ban every column of a row (n_suppress + max_len >= vocab_size)'),
 ('gitcap_student_window_beam_search: valid call',
  0,
  'student_window_beam_search: the attached constraints could ban every column of a row (n_suppress + max_len >= vocab_size)'),
 ('gitcap_student_beam_search: 1 clip x 2 beams',
  0,
  'student_window_beam_search: the attached constraints could ban every column of a row (n_suppress + max_len >= vocab_size)'),
 ('gitcap_student_greedy: all five, valid arguments',
  0,
  'student_window_beam_search: the attached constraints could ban every column of a row (n_suppress + max_len >= vocab_size)'),
 ('gitcap_student_greedy: all five, valid arguments, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_greedy: all five, a bad argument', -1, 'student_greedy: bad arguments'),
 ('gitcap_student_greedy: all five, a bad argument, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_greedy: all but the counts, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_greedy: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_window_greedy: all five, valid arguments',
  -1,
  'student_window_greedy: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_window_greedy: all five, valid arguments, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_window_greedy: all five, a bad argument',
  -1,
  'student_window_greedy: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_window_greedy: all five, a bad argument, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_window_greedy: all but the counts, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_window_greedy: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_greedy_draft: all five, valid arguments',
  -1,
  'student_greedy_draft: a prompt is attached (gitcap_student_attach_prompt), which a draft call does not take'),
 ('gitcap_student_greedy_draft: all five, valid arguments, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_greedy_draft: all five, a bad argument',
  -1,
  'student_greedy_draft: a prompt is attached (gitcap_student_attach_prompt), which a draft call does not take'),
 ('gitcap_student_greedy_draft: all five, a bad argument, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_greedy_draft: all but the counts, valid arguments',
  -1,
  'student_greedy_draft: a prompt is attached (gitcap_student_attach_prompt), which a draft call does not take'),
 ('gitcap_student_greedy_draft: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_window_greedy_draft: all five, valid arguments',
  -1,
  'student_window_greedy_draft: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_window_greedy_draft: all five, valid arguments, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_window_greedy_draft: all five, a bad argument',
  -1,
  'student_window_greedy_draft: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_window_greedy_draft: all five, a bad argument, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_window_greedy_draft: all but the counts, valid arguments',
  -1,
  'student_window_greedy_draft: a prompt is attached (gitcap_student_attach_prompt), which a draft call does not take'),
 ('gitcap_student_window_greedy_draft: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_window_greedy_partial: all five, valid arguments',
  -1,
  'student_window_greedy_partial: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_window_greedy_partial: all five, valid arguments, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_window_greedy_partial: all five, a bad argument',
  -1,
  'student_window_greedy_partial: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_window_greedy_partial: all five, a bad argument, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_window_greedy_partial: all but the counts, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_window_greedy_partial: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_pool_greedy: all five, valid arguments',
  -1,
  'student_pool_greedy: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_pool_greedy: all five, valid arguments, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_pool_greedy: all five, a bad argument',
  -1,
  'student_pool_greedy: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_pool_greedy: all five, a bad argument, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_pool_greedy: all but the counts, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_pool_greedy: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=0 tk=0 co=0 pr=0'),
 ('gitcap_student_beam_search: all five, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_beam_search: all five, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=0 pr=0'),
 ('gitcap_student_beam_search: all five, a bad argument', -1, 'student_beam_search: bad arguments'),
 ('gitcap_student_beam_search: all five, a bad argument, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=0 pr=0'),
 ('gitcap_student_beam_search: all but the counts, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_beam_search: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=0 pr=0'),
 ('gitcap_student_window_beam_search: all five, valid arguments',
  -1,
  'student_window_beam_search: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_window_beam_search: all five, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=0 pr=0'),
 ('gitcap_student_window_beam_search: all five, a bad argument',
  -1,
  'student_window_beam_search: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_window_beam_search: all five, a bad argument, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=0 pr=0'),
 ('gitcap_student_window_beam_search: all but the counts, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_window_beam_search: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=0 pr=0'),
 ('gitcap_student_score: all five, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_score: all five, valid arguments, then', 0, 'greedy=0 fc=1 lp=1 tk=0 co=1 pr=1'),
 ('gitcap_student_score: all five, a bad argument', -1, 'student_score: T < 2 (CLS and at least one token) or ld_ids < T'),
 ('gitcap_student_score: all five, a bad argument, then', 0, 'greedy=0 fc=1 lp=1 tk=0 co=1 pr=1'),
 ('gitcap_student_score: all but the counts, valid arguments',
  0,
  'student_window_push: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_score: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=0 co=1 pr=1'),
 ('gitcap_student_set_memory: all five, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_set_memory: all five, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_set_memory: all five, a bad argument', -1, 'student_set_memory: B = 0, but frame counts of 2 clips are attached'),
 ('gitcap_student_set_memory: all five, a bad argument, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_set_memory: all but the counts, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_set_memory: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_window_reset: all five, valid arguments',
  -1,
  'student_window_reset: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_window_reset: all five, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_window_reset: all five, a bad argument',
  -1,
  'student_window_reset: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_window_reset: all five, a bad argument, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_window_reset: all but the counts, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_window_reset: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_window_push: all five, valid arguments',
  -1,
  'student_window_push: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_window_push: all five, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_window_push: all five, a bad argument',
  -1,
  'student_window_push: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_window_push: all five, a bad argument, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_window_push: all but the counts, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_window_push: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_pool_reset: all five, valid arguments',
  -1,
  'student_pool_reset: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_pool_reset: all five, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_pool_reset: all five, a bad argument',
  -1,
  'student_pool_reset: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_pool_reset: all five, a bad argument, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_pool_reset: all but the counts, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_pool_reset: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_pool_push: all five, valid arguments',
  -1,
  'student_pool_push: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_pool_push: all five, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_pool_push: all five, a bad argument',
  -1,
  'student_pool_push: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_pool_push: all five, a bad argument, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_pool_push: all but the counts, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_pool_push: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_pool_drop: all five, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_pool_drop: all five, valid arguments, then', 0, 'greedy=0 fc=1 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_pool_drop: all five, a bad argument', -1, 'student_pool_drop: stream outside the pool'),
 ('gitcap_student_pool_drop: all five, a bad argument, then', 0, 'greedy=0 fc=1 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_pool_drop: all but the counts, valid arguments',
  0,
  'student_window_push: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_pool_drop: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_pool_counts: all five, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_pool_counts: all five, valid arguments, then', 0, 'greedy=0 fc=1 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_pool_counts: all five, a bad argument', -1, 'student_pool_counts: null counts_out'),
 ('gitcap_student_pool_counts: all five, a bad argument, then', 0, 'greedy=0 fc=1 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_pool_counts: all but the counts, valid arguments',
  0,
  'student_window_push: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_pool_counts: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_attention: all five, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_attention: all five, valid arguments, then', 0, 'greedy=0 fc=1 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_attention: all five, a bad argument',
  -1,
  'student_attention: null or misaligned output, T < 1, ld_ids < T, ld_f < mem_tokens, or layer outside [-1, layers)'),
 ('gitcap_student_attention: all five, a bad argument, then', 0, 'greedy=0 fc=1 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_attention: all but the counts, valid arguments',
  0,
  'student_window_push: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_attention: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_forward_decoder: all five, valid arguments', 0, 'student_window_push: null memory'),
 ('gitcap_student_forward_decoder: all five, valid arguments, then', 0, 'greedy=0 fc=1 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_forward_decoder: all five, a bad argument', -1, 'student_forward_decoder: null logits'),
 ('gitcap_student_forward_decoder: all five, a bad argument, then', 0, 'greedy=0 fc=1 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_forward_decoder: all but the counts, valid arguments',
  0,
  'student_window_push: per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take'),
 ('gitcap_student_forward_decoder: all but the counts, valid arguments, then', 0, 'greedy=0 fc=0 lp=1 tk=1 co=1 pr=1'),
 ('gitcap_student_pool_greedy: not finalized', -2, 'student_pool_greedy: weights not finalized'),
 ('gitcap_student_pool_greedy: not finalized, max_len 0', -1, 'student_pool_greedy: bad arguments'),
 ('gitcap_student_beam_search: not finalized', -2, 'student: weights not finalized'),
 ('gitcap_student_beam_search: not finalized, max_len 0', -1, 'student_beam_search: bad arguments'),
 ('gitcap_student_window_beam_search: not finalized', -2, 'student_window_beam_search: weights not finalized'),
 ('gitcap_student_window_beam_search: not finalized, max_len 0', -2, 'student_window_beam_search: weights not finalized'),
 ('gitcap_student_pool_greedy: not finalized, B 0', -1, 'student_pool_greedy: B outside [1, max_rows]'),
 ('gitcap_student_pool_greedy: not finalized, stop 7', -1, 'student_pool_greedy: unknown stop rule'),
 ('gitcap_student_beam_search: not finalized, k 0', -1, 'student_beam_search: bad arguments'),
 ('gitcap_student_window_beam_search: not finalized, k 0', -2, 'student_window_beam_search: weights not finalized'),
 ('gitcap_student_window_beam_search: not finalized, empty window', -2, 'student_window_beam_search: weights not finalized')]


def _compare(got, want):
    for g, w in zip(got, want):
        assert g == w, (g, w)
    assert len(got) == len(want) and len(want) > 50, (len(got), len(want))


def test_teacher_entry_point_errors():
    _compare(_teacher_observed(), TEACHER_EXPECTED)


def test_student_entry_point_errors():
    _compare(_student_observed(), STUDENT_EXPECTED)


def test_student_pool_beam_errors_and_pending_attachments():
    _compare(_student_more_observed(), STUDENT_MORE_EXPECTED)
