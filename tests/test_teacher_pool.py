"""The teacher's stream pool, the parts that need no device: the host plan (csrc/host_logic.h: pool_plan, through the
gitcap_dbg_pool_plan hook) against the numpy restatement in teacher_pool_reference.py, proof that the inputs of the GPU kernel
tests tell wrong kernels apart, the new symbols and kernels in the library, the refusal of a null handle, and TeacherStreamPool
over a stubbed library (the student's pool shares the base class; its own tests are in test_stream_pool.py)."""
import ctypes
import types

import numpy as np
import pytest
import torch

import teacher_pool_reference as R
from gitcap import _lib
from gitcap._stream import STOP_ALL_SEP, STOP_NEVER
from gitcap.streampool import StudentStreamPool, TeacherStreamPool, _StreamPool

ERR_ARG, ERR_STATE = -1, -2
NEW_SYMBOLS = ("gitcap_pool_reset", "gitcap_pool_push", "gitcap_pool_push_raw", "gitcap_pool_greedy", "gitcap_pool_beam_search",
               "gitcap_pool_drop", "gitcap_pool_counts", "gitcap_dbg_pool_plan", "gitcap_dbg_pool_scatter", "gitcap_dbg_pool_assemble")
NEW_KERNELS = (b"pool_scatter_kernel", b"pool_assemble_kernel")


def i32(v):
    return (ctypes.c_int32 * max(1, len(v)))(*v)


def lib_plan(lib, S, F, heads, counts, push, cap):
    """gitcap_dbg_pool_plan -> (rc, heads, counts, dst, src, pos, off, len, (total, longest, dense)); outputs are pre-filled with -7"""
    h, c = i32(heads), i32(counts)
    dst, src, pos = i32([-7] * len(push)), i32([-7] * (len(cap) * F)), i32([-7] * (len(cap) * F))
    off, ln, out3 = i32([-7] * len(cap)), i32([-7] * len(cap)), i32([-7] * 3)
    rc = lib.gitcap_dbg_pool_plan(S, F, h, c, i32(push) if push else None, len(push), dst, i32(cap) if cap else None, len(cap), src, pos,
                                  off, ln, out3)
    total = out3[0] if rc == 0 else 0
    return (rc, list(h)[:S], list(c)[:S], list(dst)[:len(push)], list(src)[:total], list(pos)[:total], list(off)[:len(cap)],
            list(ln)[:len(cap)], tuple(out3))


def check_history(lib, S, F, steps):
    """steps = [(push ids, caption ids)]: the hook, chained through its in/out cursors, against the reference pool."""
    ref = R.Pool(S, F)
    heads, counts = [0] * S, [0] * S
    for push, cap in steps:
        rc, heads, counts, dst, src, pos, off, ln, out3 = lib_plan(lib, S, F, heads, counts, push, cap)
        assert rc == 0, (push, cap)
        assert dst == ref.push(push), (push, cap)
        assert heads == ref.heads() and counts == ref.counts(), (push, cap)
        if cap:
            rsrc, rpos, roff, rlen, rout = ref.call(cap)
            assert (src, pos, off, ln, out3) == (rsrc, rpos, roff, rlen, rout), (push, cap)
    return ref


@pytest.fixture(scope="module")
def lib():
    return _lib.load()


# ---- the plan ---------------------------------------------------------------------------------------------------------------------

def test_an_empty_pool_filled_unevenly(lib):
    ref = check_history(lib, 4, 3, [([2], [2]), ([0, 2, 0], [0, 2]), ([3], [3, 0, 2]), ([0], [2, 0])])
    assert ref.counts() == [3, 0, 2, 1]
    _, _, _, _, out3 = ref.call([3, 0, 2])
    assert out3 == (6, 3, 0)                                            # ragged: 1, 3 and 2 frames


def test_a_stream_that_wrapped_its_ring(lib):
    ref = check_history(lib, 2, 3, [([1], []), ([1], []), ([1], [1]), ([1], [1]), ([1, 0], [1, 0])])
    src, pos, off, ln, _ = ref.call([1])
    assert src == [3 + 2, 3 + 0, 3 + 1] and pos == [0, 1, 2]              # five pushes: slots 0 and 1 were rewritten, slot 2 is the oldest


def test_one_push_gives_a_stream_two_frames_across_the_wrap(lib):
    ref = check_history(lib, 2, 3, [([0, 0], []), ([1, 0, 0], [0, 1])])
    assert ref.push([0, 1, 0]) == [1, 3 + 1, 2]
    rc, heads, counts, dst, *_ = lib_plan(lib, 2, 3, [1, 1], [3, 1], [0, 1, 0], [])
    assert rc == 0 and dst == [1, 4, 2] and heads == [0, 2] and counts == [3, 2]
    # F frames to one stream in one push is the most a push takes: every slot once
    rc, heads, counts, dst, *_ = lib_plan(lib, 2, 3, [2, 0], [3, 0], [0, 0, 0], [])
    assert rc == 0 and dst == [2, 0, 1] and heads == [2, 0]


def test_a_stream_holding_more_than_F_pushes(lib):
    steps = [([0], [0])] * 8 + [([0, 1, 0], [1, 0])]
    ref = check_history(lib, 2, 3, steps)
    assert ref.counts() == [3, 1]
    src, pos, *_ = ref.call([0])
    assert sorted(src) == [0, 1, 2] and pos == [0, 1, 2] and src[0] == ref.nxt[0]      # the oldest frame sits where the next one goes


def test_equal_counts_report_dense(lib):
    for counts, heads in (([2, 2, 2], [2, 2, 2]), ([3, 3, 3], [1, 0, 2]), ([1, 2, 1], [1, 2, 1])):
        rc, *_, off, ln, out3 = lib_plan(lib, 3, 3, heads, counts, [], [2, 0])
        assert rc == 0 and ln == [counts[2], counts[0]] and off == [0, counts[2]]
        assert out3 == (counts[2] + counts[0], max(counts[2], counts[0]), int(counts[2] == counts[0]))
    rc, *_, out3 = lib_plan(lib, 3, 3, [1, 2, 1], [1, 2, 1], [], [1, 0])
    assert rc == 0 and out3 == (3, 2, 0)
    rc, *_, out3 = lib_plan(lib, 3, 3, [1, 2, 1], [1, 2, 1], [], [1])
    assert rc == 0 and out3 == (2, 2, 1)                                # one row is always dense


def test_refusals_change_nothing(lib):
    heads, counts = [1, 0, 2], [1, 0, 3]
    bad_calls = [([], [0, 0], ERR_ARG), ([], [2, 0, 2], ERR_ARG), ([], [3], ERR_ARG), ([], [-1], ERR_ARG), ([], [0, 1], ERR_STATE),
                 ([3], [], ERR_ARG), ([-1], [], ERR_ARG), ([1, 1, 1, 1], [], ERR_ARG),
                 ([0], [0, 0], ERR_ARG), ([0], [1], ERR_STATE)]                      # a good push in front of a bad call: nothing happens
    for push, cap, want in bad_calls:
        rc, h, c, dst, src, pos, off, ln, out3 = lib_plan(lib, 3, 3, heads, counts, push, cap)
        assert rc == want, (push, cap)
        assert h == heads and c == counts and all(v == -7 for v in dst + off + ln + list(out3)), (push, cap)
        ref = R.Pool(3, 3)
        ref.order, ref.nxt = [[0], [], [2, 0, 1]], list(heads)
        with pytest.raises(R.Refused) as e:
            ref.push(push)
            ref.call(cap)
        assert e.value.state == (want == ERR_STATE), (push, cap)
    # a push makes an empty stream nameable in the same plan
    rc, h, c, dst, src, pos, off, ln, out3 = lib_plan(lib, 3, 3, heads, counts, [1], [1])
    assert rc == 0 and dst == [3] and src == [3] and c == [1, 1, 3]
    # the hook's own arguments
    for S, F, hd, ct in ((0, 3, [0], [0]), (1, 0, [0], [0]), (1, 256, [0], [0]), (1, 3, [3], [0]), (1, 3, [0], [4]), (1, 3, [-1], [0])):
        assert lib_plan(lib, S, F, hd, ct, [], [])[0] == ERR_ARG, (S, F, hd, ct)
    assert lib.gitcap_dbg_pool_plan(1, 3, None, i32([0]), None, 0, None, None, 0, None, None, None, None, i32([0] * 3)) == ERR_ARG


# ---- the inputs of the GPU kernel tests tell wrong kernels apart ------------------------------------------------------------------

def _gpu_inputs(D=8, N=2, seed=0):
    rng = np.random.default_rng(seed)
    p = R.gpu_pool()
    ring = rng.standard_normal((R.GPU_S * R.GPU_F, N, D)).astype(np.float32)
    temporal = rng.standard_normal((R.GPU_F, D)).astype(np.float32)
    return p, ring, temporal


def test_gpu_inputs_distinguish_the_order_of_a_clip_s_frames():
    p, ring, temporal = _gpu_inputs()
    p.push(R.GPU_PUSH)
    src, pos, off, ln, out3 = p.call([1, 2, 0])
    assert ln == [3, 2, 2] and out3[2] == 0
    good = R.bf16_round(R.assemble(ring, temporal, src, pos))
    newest_first = [s for r in range(3) for s in reversed(src[off[r]:off[r] + ln[r]])]
    assert not np.array_equal(good, R.bf16_round(R.assemble(ring, temporal, newest_first, pos)))
    for r in range(3):                                                  # every row of the call tells the two orders apart
        rows = slice(off[r] * 2, (off[r] + ln[r]) * 2)
        assert not np.array_equal(good[rows], R.bf16_round(R.assemble(ring, temporal, newest_first, pos))[rows]), r


def test_gpu_inputs_distinguish_clip_position_from_ring_position():
    p, ring, temporal = _gpu_inputs()
    p.push(R.GPU_PUSH)
    src, pos, off, ln, _ = p.call([1, 2, 0])
    ring_pos = [s % R.GPU_F for s in src]
    assert ring_pos != pos                                              # stream 1 wrapped: its oldest frame is not in slot 0
    assert ring_pos[off[0]:off[0] + ln[0]] != pos[off[0]:off[0] + ln[0]]
    good = R.bf16_round(R.assemble(ring, temporal, src, pos))
    assert not np.array_equal(good, R.bf16_round(R.assemble(ring, temporal, src, ring_pos)))
    assert not np.array_equal(good, R.bf16_round(R.assemble(ring, None, src, pos)))        # and a kernel that forgets the add


def test_gpu_inputs_distinguish_a_src_index_off_by_one_stream():
    p, ring, temporal = _gpu_inputs()
    before = p.counts()
    dst = p.push(R.GPU_PUSH)
    assert before == [1, 3, 0] and p.counts() == [2, 3, 2]
    assert dst == [6, 3 + 2, 1, 7, 3 + 0]                               # stream 1 goes on at its last slot and crosses the wrap
    src, pos, *_ = p.call([1, 2, 0])
    good = R.bf16_round(R.assemble(ring, temporal, src, pos))
    for shift in (R.GPU_F, -R.GPU_F):
        off_by_one = [(s + shift) % (R.GPU_S * R.GPU_F) for s in src]
        assert not np.array_equal(good, R.bf16_round(R.assemble(ring, temporal, off_by_one, pos)))
    # the scatter: a ring written through dst differs from one written through dst of the neighbouring stream, and the slots the
    # push does not address (4 of 9) keep what they held
    stage = np.random.default_rng(1).standard_normal((len(dst), 2, 8)).astype(np.float32)
    poison = np.full_like(ring, np.nan)
    out = R.scatter(poison.copy(), stage, dst)
    wrong = R.scatter(poison.copy(), stage, [(d + R.GPU_F) % 9 for d in dst])
    assert not np.array_equal(np.isnan(out), np.isnan(wrong))
    assert sorted(set(range(9)) - set(dst)) == [0, 2, 4, 8] and np.isnan(out[[0, 2, 4, 8]]).all() and not np.isnan(out[dst]).any()


# ---- the library ------------------------------------------------------------------------------------------------------------------

def test_symbols_kernels_and_null_handles(lib):
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS and hasattr(lib, name), name
    blob = open(_lib.LIB_PATH, "rb").read()
    for k in NEW_KERNELS:
        assert k in blob, k
    ids = i32([0])
    assert lib.gitcap_pool_reset(None, 1, 1) == ERR_ARG
    assert lib.gitcap_pool_push(None, None, ids, 1, None) == ERR_ARG
    assert lib.gitcap_pool_push_raw(None, None, ids, 1, 4, 4, None) == ERR_ARG
    assert lib.gitcap_pool_greedy(None, ids, 1, 4, 0, None, None, None, None) == ERR_ARG
    assert b"pool_greedy: null handle" in lib.gitcap_last_error(None)
    assert lib.gitcap_pool_beam_search(None, ids, 1, 2, 4, ctypes.c_float(0.6), 2, None, None, None) == ERR_ARG
    assert lib.gitcap_pool_drop(None, 0) == ERR_ARG and lib.gitcap_pool_counts(None, ids) == ERR_ARG
    assert lib.gitcap_abi_version() == 1


# ---- TeacherStreamPool over a stubbed library -------------------------------------------------------------------------------------

CLS, SEP, F, MAXB, L = 7, 9, 3, 2, 5


class _Pool(TeacherStreamPool):
    """The library's side replaced: a stream's caption is CLS, its id, the frames it holds, SEP, SEP (so every row's cut differs
    from the batch's when the rows' SEPs would), and every call is logged."""

    def __init__(self, streams, hop=1, min_frames=1, mode=STOP_ALL_SEP, beam=None):
        self.log, self.ref = [], R.Pool(streams, F)
        model = types.SimpleNamespace(max_batch=MAXB, cfg=types.SimpleNamespace(sep_token_id=SEP), _dev="cpu", _pool_owner=None,
                                      poll_errors=lambda: self.log.append("poll"))
        super().__init__(model, streams, F, hop, L, mode, True, 0, min_frames, (None, None), beam)

    def _reset_lib(self):
        self.log.append(("reset", self._sched.streams, self._sched.window))

    def _prepare(self, frames):
        return frames, False

    def _push_lib(self, prepared, ids):
        self.log.append(("push", list(ids)))
        self.ref.push(ids)

    def _drop_lib(self, s):
        self.ref.order[s], self.ref.nxt[s] = [], 0

    def _counts_lib(self):
        return self.ref.counts()

    def _caption_lib(self, ids):
        self.log.append(("caption", list(ids)))
        held = self.ref.counts()
        seen = [held[s] for s in ids]
        if self._beam is not None:
            return (torch.tensor([[CLS, s, SEP, SEP, SEP] for s in ids]), torch.tensor([-float(s) for s in ids])), None, None, seen
        rows = torch.tensor([[CLS, s, 20 + held[s]] + ([SEP, SEP, 1] if s % 2 else [3, SEP, 1]) for s in ids])
        return rows, torch.arange(len(ids) * L, dtype=torch.float32).view(len(ids), L), None, seen


def test_the_two_pools_share_one_base_class():
    assert issubclass(TeacherStreamPool, _StreamPool) and issubclass(StudentStreamPool, _StreamPool)
    for name in ("push", "caption", "_caption", "drop", "counts", "_check_live"):
        assert name not in vars(StudentStreamPool), name                # the student's pool is the base plus its library calls
        assert getattr(StudentStreamPool, name) is getattr(_StreamPool, name)


def test_schedule_chunks_and_cuts_over_a_stubbed_library():
    p = _Pool(5, hop=2, min_frames=2)
    assert p.log == [("reset", 5, F)]
    fr = torch.zeros(3, 1)
    assert sorted(p.push(fr, [0, 1, 0])) == [0]                         # stream 0 holds two frames and saw two: due; stream 1 is not
    assert ("caption", [0]) in p.log and ("caption", [1]) not in p.log
    out = p.push(torch.zeros(5, 1), [1, 2, 2, 3, 3])                    # 1, 2, 3 due: chunks of max_batch = 2
    assert [e for e in p.log if e != "poll"][-2:] == [("caption", [1, 2]), ("caption", [3])] and sorted(out) == [1, 2, 3]
    assert out[1].tolist() == [CLS, 1, 22, SEP] and out[2].tolist() == [CLS, 2, 22, 3, SEP]         # each row cut at its OWN first SEP
    assert p.last_logprobs[1].tolist() == [0.0, 1.0, 2.0] and p.last_logprobs[2].tolist() == [5.0, 6.0, 7.0, 8.0]
    assert p.last_frames == {0: 2, 1: 2, 2: 2, 3: 2} and "poll" in p.log                            # CPU frames in: vouched for
    with pytest.raises(ValueError, match="at most 3 frames per stream"):
        p.push(torch.zeros(4, 1), [4] * 4)
    with pytest.raises(ValueError, match="at most max_batch \\* frames = 6 frames"):
        p.push(torch.zeros(7, 1), [0, 1, 2, 3, 4, 0, 1])
    with pytest.raises(ValueError, match="named twice"):
        p.caption([1, 1])
    p.drop(1)
    assert p.counts()[1] == 0 and 1 not in p.last_frames and 1 not in p.last_logprobs
    never = _Pool(2, mode=STOP_NEVER)
    assert never.push(fr[:1], [1])[1].tolist() == [CLS, 1, 21, SEP, SEP, 1]
    p2 = _Pool(1)                                                       # a second pool on another model leaves p alone ...
    p.counts()
    p._m._pool_owner = p2._token                                       # ... one on the same model invalidates it
    with pytest.raises(_lib.GitcapError, match="this _Pool was invalidated"):
        p.counts()


def test_a_beam_pool_returns_predictions_and_scores():
    p = _Pool(3, beam=(2, 0.6, 2))
    out = p.push(torch.zeros(2, 1), [2, 0])
    assert out[2].tolist() == [CLS, 2, SEP, SEP, SEP] and float(p.last_scores[2]) == -2.0 and p.last_frames == {0: 1, 2: 1}
    p.drop(2)
    assert 2 not in p.last_scores
