"""The student's stream pool, the parts that need no device: the per-stream schedule (hop and min_frames per stream), the chunking
of the due streams, the cut at a row's own first SEP -- StudentStreamPool with its library calls stubbed --, the declarations
in include/gitcap.h, the exported symbols, the refusal of a null handle before any device is touched, and the two new kernels in
the gfx950 code object.  The device tests are in test_stream_pool_gpu.py and test_stream_pool_e2e_gpu.py."""
import ctypes
import os
import re
import types

import pytest
import torch

from gitcap import _lib
from gitcap._stream import STOP_ALL_SEP, STOP_NEVER
from gitcap.streampool import StudentStreamPool, cut_at_sep
from gitcap.window import PoolSchedule

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("gitcap_student_pool_reset", "gitcap_student_pool_push", "gitcap_student_pool_greedy", "gitcap_student_pool_drop",
               "gitcap_student_pool_counts")
NEW_KERNELS = ("student_pool_scatter_kernel", "student_pool_gather_kernel")
CLS, SEP, F, D, MAXB, L = 7, 9, 4, 8, 3, 5


# ---- the schedule ---------------------------------------------------------------------------------------------------------------

def test_schedule_counts_hop_and_min_frames_per_stream():
    s = PoolSchedule(3, window=F, hop=2, min_frames=3)
    assert s.push([0]) == [] and s.push([0, 1]) == []                   # stream 0: two frames arrived, but it holds fewer than three
    assert s.push([1, 0, 1]) == [0, 1]                                  # both hold three and saw >= 2 since their last caption
    s.captioned([0])
    assert s.push([2]) == [1]                                           # 1 stays due until it is captioned; 2 holds one frame
    s.captioned([1])
    assert s.push([0]) == [] and s.push([0]) == [0]                     # hop counts from the stream's own last caption
    assert s.held == [F, 3, 1]                                          # a window never holds more than `window`
    s.drop(0)
    assert s.held[0] == 0 and s.since[0] == 0 and s.push([0, 0]) == []
    for bad, msg in (([], "at least one frame"), ([3], "stream 3 outside 0..2"), ([-1], "stream -1 outside"), ([1] * (F + 1), "at most 4 frames per stream, got 5 for stream 1")):
        before = (list(s.held), list(s.since))
        with pytest.raises(ValueError, match=msg):
            s.push(bad)
        assert (s.held, s.since) == before
    for kw in (dict(streams=0), dict(hop=0), dict(min_frames=0), dict(min_frames=F + 1)):
        with pytest.raises(ValueError):
            PoolSchedule(**{**dict(streams=2, window=F, hop=1, min_frames=1), **kw})
    full = PoolSchedule(1, window=F, hop=1, min_frames=F)               # min_frames = window: nothing before the window is full
    assert [full.push([0]) for _ in range(F + 1)] == [[]] * (F - 1) + [[0], [0]]


def test_cut_at_a_row_s_own_first_sep():
    row = lambda *t: torch.tensor((CLS,) + t)
    assert cut_at_sep(row(3, SEP, 4, SEP), SEP) == 2
    assert cut_at_sep(row(SEP, 1, 1, 1), SEP) == 1
    assert cut_at_sep(row(1, 2, 3, 4), SEP) == 4
    assert cut_at_sep(torch.tensor([SEP, 1, SEP]), SEP) == 2            # column 0 is CLS whatever it holds


# ---- StudentStreamPool over a stubbed library -------------------------------------------------------------------------------------

class _Pool(StudentStreamPool):
    """The library calls replaced: a stream's caption is a function of (stream, frames held), whatever shares its call."""

    def __init__(self, *a, **k):
        self.calls = []
        super().__init__(*a, **k)

    def _reset_lib(self):
        self.calls.append(("reset", self._sched.streams))

    def _push_lib(self, mem, ids):
        self.calls.append(("push", tuple(mem.shape), tuple(ids)))

    def _drop_lib(self, s):
        self.calls.append(("drop", s))

    def _counts_lib(self):
        return list(self._sched.held)

    def _caption_lib(self, ids):
        self.calls.append(("caption", tuple(ids)))
        assert 1 <= len(ids) <= MAXB and len(set(ids)) == len(ids)
        rows = torch.full((len(ids), L + 1), 1, dtype=torch.int64)
        rows[:, 0] = CLS
        for r, s in enumerate(ids):
            rows[r, 1 + s % L] = SEP                                     # stream s emits SEP as its (s % L + 1)-th token ...
            rows[r, 1 + s % L + 1:] = 50 + s                             # ... and what lies behind depends on nothing the pool keeps
        lp = -torch.arange(L, dtype=torch.float32).repeat(len(ids), 1) - torch.tensor(ids, dtype=torch.float32)[:, None] if self._want_lp else None
        tk = None
        if self._top_k:
            tk = (rows[:, 1:, None].repeat(1, 1, self._top_k), torch.zeros(len(ids), L, self._top_k))
        return rows, lp, tk, [self._sched.held[s] for s in ids]


def _model():
    m = types.SimpleNamespace(cfg=types.SimpleNamespace(mem_tokens=F, d_model=D, sep_token_id=SEP), max_batch=MAXB, _dev=torch.device("cpu"),
                              _pool_owner=None, _window_owner="a live caption_stream")
    m._native = lambda: False
    return m


def test_pool_chunks_the_due_streams_and_cuts_each_row_at_its_own_sep():
    m = _model()
    p = _Pool(m, 5, 1, L, STOP_ALL_SEP, True, 2, 1)
    assert p.calls == [("reset", 5)] and m._window_owner == "a live caption_stream"      # opening a pool leaves the stream's token alone
    out = p.push(torch.zeros(5, D), [4, 0, 3, 1, 2])
    assert p.calls[1:] == [("push", (5, D), (4, 0, 3, 1, 2)), ("caption", (0, 1, 2)), ("caption", (3, 4))]      # chunks of max_batch
    assert sorted(out) == [0, 1, 2, 3, 4]
    for s, ids in out.items():
        assert ids.tolist() == [CLS] + [1] * (s % L) + [SEP], s          # behind its own first SEP, not the batch's last
        assert p.last_logprobs[s].tolist() == [-float(t) - s for t in range(s % L + 1)]
        assert p.last_top_ids[s].shape == (s % L + 1, 2) and p.last_top_logprobs[s].shape == (s % L + 1, 2)
        assert p.last_frames[s] == 1
    # a stream's result does not depend on who else was due
    alone = p.caption([3])
    assert alone[3].tolist() == out[3].tolist() and p.calls[-1] == ("caption", (3,))
    with pytest.raises(ValueError, match="named twice"):
        p.caption([1, 1])
    # stop = never: whole rows
    q = _Pool(m, 2, 1, L, STOP_NEVER, False, 0, 1)
    got = q.push(torch.zeros(1, D), [1])
    assert got[1].tolist() == [CLS, 1, SEP, 51, 51, 51] and q.last_logprobs == {} and q.last_frames == {1: 1}
    with pytest.raises(_lib.GitcapError, match="this _Pool was invalidated"):
        p.push(torch.zeros(1, D), [0])                                    # q took the pool over


def test_pool_schedule_hop_min_frames_drop_and_refusals():
    m = _model()
    p = _Pool(m, 3, 2, L, STOP_ALL_SEP, False, 0, 2)
    assert p.push(torch.zeros(1, D), [1]) == {}
    assert sorted(p.push(torch.zeros(3, D), [1, 0, 2])) == [1]            # stream 1: two frames; 0 and 2 hold one
    assert p.push(torch.zeros(1, D), [1]) == {}                           # hop = 2: one frame since its caption
    assert sorted(p.push(torch.zeros(2, D), [1, 0])) == [0, 1]
    p.drop(1)
    assert p._sched.held == [2, 0, 1] and 1 not in p.last_frames
    assert p.push(torch.zeros(1, D), [1]) == {}                           # starts again below min_frames
    n = len(p.calls)
    with pytest.raises(ValueError, match="2 frames for 1 stream ids"):
        p.push(torch.zeros(2, D), [0])
    with pytest.raises(ValueError, match="stream 3 outside"):
        p.push(torch.zeros(1, D), [3])
    with pytest.raises(ValueError, match=r"expected memory tokens \[n,8\]"):
        p.push(torch.zeros(1, D + 1), [0])
    with pytest.raises(_lib.GitcapError, match=r"needs the native TinyViT encoder \(image_encoder='native'\)"):
        p.push(torch.zeros(1, 6, 6, 3, dtype=torch.uint8), [0])           # camera frames, and the model has no native encoder
    with pytest.raises(ValueError, match="stream 7 outside"):
        p.drop(7)
    assert len(p.calls) == n and p._sched.held == [2, 1, 1]               # refused before any library call or bookkeeping
    m._pool_owner = None                                                  # what a moved model does
    with pytest.raises(_lib.GitcapError, match="was invalidated"):
        p.counts()


def test_stream_pool_checks_its_arguments_before_any_library_call():
    from gitcap.student import StudentCaptioner
    fake = types.SimpleNamespace(max_text_len=8, stop="all_sep")
    for kw, msg in ((dict(streams=0), "streams=0 outside"), (dict(streams=4097), "streams=4097 outside"), (dict(streams=2, max_len=9), "max_len=9 outside"),
                    (dict(streams=2, top_logprobs=33), "top_logprobs=33 outside")):
        with pytest.raises(ValueError, match=msg):
            StudentCaptioner.stream_pool(fake, **kw)


# ---- header, library ------------------------------------------------------------------------------------------------------------

def test_symbols_are_declared_bound_and_exported():
    header = open(os.path.join(ROOT, "include", "gitcap.h")).read()
    for name in NEW_SYMBOLS:
        assert re.search(r"^int %s\(" % name, header, re.M), name
        assert name in _lib.SYMBOLS, name
    assert "int gitcap_student_pool_counts(const gitcap_student_t* h, int32_t* counts_out);" in header
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name), name
    lib.gitcap_abi_version.restype = ctypes.c_int
    assert lib.gitcap_abi_version() == 1                                  # new symbols only
    blob = open(_lib.LIB_PATH, "rb").read()
    for kernel in NEW_KERNELS:
        assert kernel.encode() in blob, kernel


def test_null_handle_is_refused_without_a_device():
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()                                          # a non-null host pointer: must never be dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)
    i32 = ctypes.cast(buf, ctypes.POINTER(ctypes.c_int32))
    assert lib.gitcap_student_pool_reset(None, 2) == -1
    assert lib.gitcap_student_pool_push(None, p, i32, 1, None) == -1
    assert lib.gitcap_student_pool_greedy(None, i32, 1, 4, 0, p, p, i32, None) == -1
    assert lib.gitcap_student_pool_drop(None, 0) == -1
    assert lib.gitcap_student_pool_counts(None, i32) == -1
    assert b"null handle" in lib.gitcap_student_last_error(None)
