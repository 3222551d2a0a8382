"""The student's stream pool through the C ABI (include/gitcap.h: gitcap_student_pool_*), memory tokens as input.  The contract is
exact: a stream's row of gitcap_student_pool_greedy holds, bit for bit, what gitcap_student_greedy yields on that stream's current
tokens (kept by the tests on the host, oldest first) with their counts attached -- ids, log-probabilities and alternatives --
whichever streams share the call, wherever the stream's ring has wrapped to."""
import ctypes

import pytest
import torch

from gitcap import _lib
from gpu_support import NAN, assert_tail, make_student, poisoned, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

L, TK = 6, 3                    # max_len, alternatives per step
IDS_FILL = -777
ERR_ARG, ERR_STATE = -1, -2
KW = dict(max_batch=4, max_text_len=8, stop="never")


def c32(v):
    return (ctypes.c_int32 * len(v))(*v)


@pytest.fixture(scope="module")
def st():
    assert torch.cuda.is_available()
    return make_student("tiny", **KW)


def tokens(n, D, seed):
    return 2.0 * torch.randn(n, D, generator=torch.Generator().manual_seed(seed))


class Out:
    """Poisoned output buffers of one greedy call over `rows` rows, one row longer than the call may write."""

    def __init__(self, rows):
        self.rows = rows
        self.ids = poisoned((rows + 1, L + 1), IDS_FILL, torch.int64)
        self.lp = poisoned((rows + 1, L), NAN)
        self.tk_ids = poisoned((rows + 1, L, TK), IDS_FILL, torch.int64)
        self.tk_lp = poisoned((rows + 1, L, TK), NAN)

    def attach(self, m):
        m._call("gitcap_student_attach_token_logprobs", _lib.ptr(self.lp), L)
        m._call("gitcap_student_attach_top_logprobs", TK, _lib.ptr(self.tk_ids), _lib.ptr(self.tk_lp), L)

    def untouched(self, used_rows):
        for buf, per, fill in ((self.ids, L + 1, IDS_FILL), (self.lp, L, NAN), (self.tk_ids, L * TK, IDS_FILL), (self.tk_lp, L * TK, NAN)):
            assert_tail(buf, used_rows * per, fill)

    def result(self):
        torch.cuda.synchronize()
        self.untouched(self.rows)
        r = self.rows
        return self.ids[:r].clone(), self.lp[:r].clone(), self.tk_ids[:r].clone(), self.tk_lp[:r].clone()


def same(got, ref, what):
    for g, r, name in zip(got, ref, ("ids", "logprobs", "top ids", "top logprobs")):
        assert g.shape == r.shape, (what, name)
        assert torch.equal(g, r) if g.dtype == torch.int64 else same_bits(g.contiguous(), r.contiguous()), (what, name)


def rows_of(res, rows):
    return tuple(t[rows] for t in res)


def pool_push(m, mem, ids):
    mem = mem.cuda().contiguous()
    m._call("gitcap_student_pool_push", _lib.ptr(mem), c32(ids), len(ids), m._stream())


def pool_greedy(m, ids):
    """-> ((ids, logprobs, top ids, top logprobs) of the named streams, frames_out)"""
    o = Out(len(ids))
    o.attach(m)
    seen = c32([-1] * len(ids))
    m._call("gitcap_student_pool_greedy", c32(ids), len(ids), L, 0, _lib.ptr(o.ids), None, seen, m._stream())
    return o.result(), list(seen)


def pool_counts(m, S):
    out = c32([-1] * S)
    m._call("gitcap_student_pool_counts", out)
    return list(out)


def ref_greedy(m, windows):
    """gitcap_student_greedy with gitcap_student_attach_frame_counts on these windows ([n_b, D] each, oldest first), packed."""
    o = Out(len(windows))
    packed = torch.cat(windows, 0).cuda().contiguous()
    m._call("gitcap_student_attach_frame_counts", c32([w.shape[0] for w in windows]), len(windows))
    o.attach(m)
    m._call("gitcap_student_greedy", _lib.ptr(packed), len(windows), L, 0, _lib.ptr(o.ids), None, m._stream())
    return o.result()


class HostPool:
    """What the test keeps beside the device's pool: every stream's tokens in arrival order."""

    def __init__(self, m, S):
        self.m, self.F = m, m.cfg.mem_tokens
        self.seen = [[] for _ in range(S)]
        m._call("gitcap_student_pool_reset", S)

    def push(self, mem, ids):
        pool_push(self.m, mem, ids)
        for t, s in zip(mem, ids):
            self.seen[s].append(t)

    def window(self, s):
        return torch.stack(self.seen[s][-self.F:], 0)

    def counts(self):
        return [min(len(t), self.F) for t in self.seen]


def mixed_pool(m):
    """5 streams behind interleaved pushes: stream 0 holds F + 2 pushed tokens (wrapped), 1 exactly F, 2 one, 3 F - 1, 4 none.
    Several streams per push, out of order inside a push."""
    F, D = m.cfg.mem_tokens, m.cfg.d_model
    hp = HostPool(m, 5)
    order = [0] * (F + 2) + [1] * F + [2] + [3] * (F - 1)
    perm = torch.randperm(len(order), generator=torch.Generator().manual_seed(5)).tolist()
    order = [order[i] for i in perm]
    mem = tokens(len(order), D, 11)
    at, sizes, unsorted = 0, [5, 1, F, 2, 3], 0
    while at < len(order):
        n = min(sizes[0], len(order) - at)
        sizes = sizes[1:] + sizes[:1]
        hp.push(mem[at:at + n], order[at:at + n])
        unsorted += order[at:at + n] != sorted(order[at:at + n])
        at += n
    assert [len(t) for t in hp.seen] == [F + 2, F, 1, F - 1, 0] and unsorted >= 2
    return hp


def test_mixed_fill_levels_unsorted_call(st):
    F = st.cfg.mem_tokens
    hp = mixed_pool(st)
    assert pool_counts(st, 5) == [F, F, 1, F - 1, 0] == hp.counts()
    call = [3, 0, 2, 1]
    got, seen = pool_greedy(st, call)
    assert seen == [F - 1, F, 1, F]
    same(got, ref_greedy(st, [hp.window(s) for s in call]), "pool against the full call with counts")


def test_a_stream_alone_is_the_stream_in_the_batch(st):
    hp = mixed_pool(st)
    call = [3, 0, 2, 1]
    batch, _ = pool_greedy(st, call)
    for r, s in enumerate(call):
        alone, seen = pool_greedy(st, [s])
        assert seen == [hp.counts()[s]]
        same(alone, rows_of(batch, slice(r, r + 1)), f"stream {s} alone")


def window_partial(m, B):
    o = Out(B)
    m._call("gitcap_student_attach_token_logprobs", _lib.ptr(o.lp), L)
    seen = ctypes.c_int32(-1)
    m._call("gitcap_student_window_greedy_partial", L, 0, _lib.ptr(o.ids), None, ctypes.byref(seen), m._stream())
    torch.cuda.synchronize()
    assert_tail(o.ids, B * (L + 1), IDS_FILL)
    assert_tail(o.lp, B * L, NAN)
    return (o.ids[:B].clone(), o.lp[:B].clone()), int(seen.value)


def test_one_stream_through_two_wraps(st):
    F, D = st.cfg.mem_tokens, st.cfg.d_model
    hp = HostPool(st, 3)
    st._call("gitcap_student_window_reset", 1)
    mem, other = tokens(2 * F + 1, D, 21), tokens(4 * F + 2, D, 22)
    for i in range(2 * F + 1):
        # the stream's token between two tokens of the other streams, in one push
        hp.push(torch.stack([other[2 * i], mem[i], other[2 * i + 1]], 0), [i % 2, 2, (i + 1) % 2])
        one = mem[i:i + 1].cuda().contiguous()
        st._call("gitcap_student_window_push", _lib.ptr(one), 1, 1, st._stream())
        want, wseen = window_partial(st, 1)
        got, seen = pool_greedy(st, [2])
        assert seen == [wseen] == [min(i + 1, F)]
        same(got[:2], want, f"after {i + 1} pushes")
    st._call("gitcap_student_window_reset", 0)


def test_all_full_is_the_lockstep_window(st):
    F, D = st.cfg.mem_tokens, st.cfg.d_model
    mem = tokens(3 * F, D, 31).view(3, F, D)
    hp = HostPool(st, 3)
    for f in range(F):                                  # stream b's token f = clip b's token f, the streams in another order each time
        order = [(f + j) % 3 for j in range(3)]
        hp.push(torch.stack([mem[b, f] for b in order], 0), order)
    st._call("gitcap_student_window_reset", 3)
    dev = mem.cuda().contiguous()
    st._call("gitcap_student_window_push", _lib.ptr(dev), 3, F, st._stream())
    o = Out(3)
    o.attach(st)
    st._call("gitcap_student_window_greedy", L, 0, _lib.ptr(o.ids), None, st._stream())
    want = o.result()
    got, seen = pool_greedy(st, [0, 1, 2])
    assert seen == [F, F, F]
    same(got, want, "three full streams against a lockstep window of three")
    st._call("gitcap_student_window_reset", 0)


def test_window_and_pool_on_one_handle(st):
    F, D = st.cfg.mem_tokens, st.cfg.d_model
    hp = HostPool(st, 3)
    st._call("gitcap_student_window_reset", 2)
    wmem, pmem = tokens(2 * (F + 1), D, 41).view(2, F + 1, D), tokens(3 * (F + 1), D, 42)
    for i in range(F + 1):
        one = wmem[:, i:i + 1].cuda().contiguous()
        st._call("gitcap_student_window_push", _lib.ptr(one), 2, 1, st._stream())
        hp.push(pmem[3 * i:3 * i + 3], [2, 0, 2] if i % 2 else [1, 2, 0])
        n = min(i + 1, F)
        want = ref_greedy(st, [wmem[b, i + 1 - n:i + 1] for b in range(2)])
        got, seen = window_partial(st, 2)
        assert seen == n
        same(got, want[:2], f"the window after {i + 1} pushes beside a pool")
        call = [s for s in (2, 0, 1) if hp.seen[s]]
        pgot, pseen = pool_greedy(st, call)
        assert pseen == [hp.counts()[s] for s in call]
        same(pgot, ref_greedy(st, [hp.window(s) for s in call]), f"the pool after {i + 1} pushes beside a window")
    counts = pool_counts(st, 3)
    st._call("gitcap_student_window_reset", 0)          # releasing the window leaves the pool alone, and the reverse
    assert pool_counts(st, 3) == counts == hp.counts()
    st._call("gitcap_student_window_reset", 1)
    st._call("gitcap_student_pool_reset", 0)
    one = wmem[:1, :1].cuda().contiguous()
    st._call("gitcap_student_window_push", _lib.ptr(one), 1, 1, st._stream())
    got, seen = window_partial(st, 1)
    same(got, ref_greedy(st, [wmem[0, :1]])[:2], "the window after the pool was released")
    st._call("gitcap_student_window_reset", 0)


def test_drop_empties_one_stream(st):
    F = st.cfg.mem_tokens
    hp = mixed_pool(st)
    before, _ = pool_greedy(st, [0, 2, 3])
    st._call("gitcap_student_pool_drop", 1)
    assert pool_counts(st, 5) == [F, 0, 1, F - 1, 0]
    after, _ = pool_greedy(st, [0, 2, 3])
    same(after, before, "the other streams behind a drop")
    o = Out(2)
    o.attach(st)
    rc = st._lib.gitcap_student_pool_greedy(st._handle, c32([0, 1]), 2, L, 0, _lib.ptr(o.ids), None, None, st._stream())
    torch.cuda.synchronize()
    assert rc == ERR_STATE and b"stream 1 holds no token" in st._lib.gitcap_student_last_error(st._handle)
    o.untouched(0)
    # the dropped stream starts again from its first slot
    mem = tokens(2, st.cfg.d_model, 51)
    hp.seen[1] = []
    hp.push(mem, [1, 1])
    got, seen = pool_greedy(st, [1, 0])
    assert seen == [2, F]
    same(got, ref_greedy(st, [hp.window(1), hp.window(0)]), "a stream pushed again behind its drop")


def test_refusals_change_nothing(st):
    F, D, R = st.cfg.mem_tokens, st.cfg.d_model, KW["max_batch"]
    hp = mixed_pool(st)
    counts = hp.counts()
    lib, h, s = st._lib, st._handle, st._stream()
    mem = tokens(F + 1, D, 61).cuda().contiguous()
    err = lambda: lib.gitcap_student_last_error(h)
    # pushes: more than F tokens for one stream, ids outside the pool
    assert lib.gitcap_student_pool_push(h, _lib.ptr(mem), c32([2] * (F + 1)), F + 1, s) == ERR_ARG and b"more than mem_tokens" in err()
    assert lib.gitcap_student_pool_push(h, _lib.ptr(mem), c32([0, -1]), 2, s) == ERR_ARG and b"names stream -1" in err()
    assert lib.gitcap_student_pool_push(h, _lib.ptr(mem), c32([0, 1, 5]), 3, s) == ERR_ARG and b"names stream 5" in err()
    assert lib.gitcap_student_pool_push(h, _lib.ptr(mem), c32([0]), 0, s) == ERR_ARG
    assert lib.gitcap_student_pool_push(h, _lib.ptr(mem), c32([0]), R * F + 1, s) == ERR_ARG
    assert pool_counts(st, 5) == counts
    before, _ = pool_greedy(st, [0, 1, 2, 3])           # (the refused pushes wrote no slot either)
    same(before, ref_greedy(st, [hp.window(i) for i in range(4)]), "behind the refused pushes")
    # calls
    def refused(ids, B, code, msg, attach_counts=False):
        o = Out(R + 1)
        o.attach(st)
        if attach_counts:
            st._call("gitcap_student_attach_frame_counts", c32([1, 1]), 2)
        seen = c32([-9] * (R + 1))
        rc = lib.gitcap_student_pool_greedy(h, c32(ids), B, L, 0, _lib.ptr(o.ids), None, seen, s)
        torch.cuda.synchronize()
        assert rc == code and msg in err(), (rc, err())
        o.untouched(0)
        assert list(seen) == [-9] * (R + 1)
    refused([0, 1, 0], 3, ERR_ARG, b"stream 0 is named twice")
    refused([0, -1], 2, ERR_ARG, b"names stream -1")
    refused([5], 1, ERR_ARG, b"names stream 5")
    refused([0, 1, 2, 3, 4], R + 1, ERR_ARG, b"B outside [1, max_rows]")
    refused([0, 4], 2, ERR_STATE, b"stream 4 holds no token")
    refused([0, 1], 2, ERR_ARG, b"per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take",
            attach_counts=True)
    assert lib.gitcap_student_pool_drop(h, 5) == ERR_ARG and lib.gitcap_student_pool_drop(h, -1) == ERR_ARG
    assert lib.gitcap_student_pool_reset(h, 4097) == ERR_ARG and lib.gitcap_student_pool_reset(h, -1) == ERR_ARG
    assert pool_counts(st, 5) == counts
    after, _ = pool_greedy(st, [0, 1, 2, 3])            # nothing stayed attached, nothing moved
    same(after, before, "behind the refused calls")
    # no pool
    st._call("gitcap_student_pool_reset", 0)
    refused([0], 1, ERR_STATE, b"no pool")
    assert lib.gitcap_student_pool_push(h, _lib.ptr(mem), c32([0]), 1, s) == ERR_STATE and b"no pool" in err()
    assert lib.gitcap_student_pool_counts(h, c32([0] * 5)) == ERR_STATE
    assert lib.gitcap_student_pool_drop(h, 0) == ERR_STATE
