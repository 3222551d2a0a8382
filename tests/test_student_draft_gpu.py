"""Student greedy decoding that verifies a draft caption in one pass (gitcap_student_greedy_draft / _window_greedy_draft,
StudentCaptioner.greedy_decode(draft=...), caption_stream(carry=True)).

Every comparison is torch.equal against the plain call with the same arguments: the draft path is defined as bitwise equal to it,
whatever the draft holds, and the plain call is held to the oracle by tests/test_student.py."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch

from gitcap.student_config import student_synthetic_weights, student_tiny
from gpu_support import make_student, make_student_native, ptr, student_cfg
from oracle.student_oracle import StudentOracle, make_memory

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -1, -2
STOP_NEVER, STOP_ALL_SEP = 0, 1
MAX_B, MAX_T = 5, 25


_MODELS, _REFS = {}, {}


def _model(name):
    """One model per size for the whole module (max_batch 5, max_text_len 25)."""
    if name not in _MODELS:
        _MODELS[name] = make_student(name, max_batch=MAX_B, max_text_len=MAX_T)
    return _MODELS[name]


def _ref(name, B, max_len):
    """(memory on the device, plain greedy ids under stop='never', the same for another memory): computed once per case."""
    key = (name, B, max_len)
    if key not in _REFS:
        m, cfg = _model(name), student_cfg(name)
        mem = make_memory(B, cfg.mem_tokens, cfg.d_model, 40 + B).cuda()
        other = make_memory(B, cfg.mem_tokens, cfg.d_model, 90 + B).cuda()
        _REFS[key] = (mem, m.greedy_decode(mem, max_len=max_len, stop="never").clone(),
                      m.greedy_decode(other, max_len=max_len, stop="never").clone())
    return _REFS[key]


def _changed(ref, cols, V):
    """ref with the token of row r at column cols[r] replaced by another word."""
    d = ref.clone()
    for r, c in enumerate(cols):
        d[r, c] = (d[r, c] + 1) % V
    return d


def _drafts(cfg, ref, other_ids, max_len):
    B, V = ref.shape[0], cfg.vocab_length
    g = torch.Generator().manual_seed(7)
    oov = ref.clone()
    oov[0, 2] = V + 7
    oov[B - 1, min(5, max_len)] = -1
    return [
        ("ref", ref),
        ("col 1", _changed(ref, [1] * B, V)),
        ("col mid", _changed(ref, [max_len // 2] * B, V)),
        ("col last", _changed(ref, [max_len] * B, V)),
        ("col per row", _changed(ref, [1 + (3 * r + 2) % max_len for r in range(B)], V)),
        ("short", ref[:, :4]),
        ("random", torch.randint(0, V, (B, max_len + 1), generator=g).to(ref.device)),
        ("all PAD", torch.full_like(ref, cfg.pad_token_id)),
        ("all SEP", torch.full_like(ref, cfg.sep_token_id)),
        ("outside the vocabulary", oov),
        ("another memory", other_ids),
    ]


def _expected_accept(ref, d):
    """min over the rows of the common prefix of d[:, 1:] and ref[:, 1:1+n]."""
    n = d.shape[1] - 1
    same = (d[:, 1:] == ref[:, 1:1 + n]).long().cumprod(dim=1).sum(dim=1)
    return int(same.min())


CASES = [(name, B, L) for name in ("tiny", "base") for B in (1, 2, 3, 5) for L in (8, 25)]


# ---------------------------------------------------------------------------------------------------- 1. equality under every draft
@pytest.mark.gpu
@pytest.mark.parametrize("stop", ["never", "all_sep"])
@pytest.mark.parametrize("name,B,max_len", CASES)
def test_gpu_draft_never_changes_the_result(name, B, max_len, stop):
    """B = 1, 2: the token steps take the one/two-row prologue of skinny.hip and the verify pass (n_draft >= 3) does not."""
    m, cfg = _model(name), student_cfg(name)
    mem, ref, other_ids = _ref(name, B, max_len)
    want = m.greedy_decode(mem, max_len=max_len, stop=stop).clone()
    if stop == "never":
        assert torch.equal(want, ref)
    for label, d in _drafts(cfg, ref, other_ids, max_len):
        got = m.greedy_decode(mem, max_len=max_len, stop=stop, draft=d)
        assert got.device == want.device and torch.equal(got, want), (label, got.tolist(), want.tolist())
        assert torch.equal(m.greedy_decode(mem, max_len=max_len, stop=stop, draft=d.cpu()), want), label   # a CPU draft
    assert torch.equal(m.greedy_decode(mem, max_len=max_len, stop=stop), want)          # the plain call afterwards


# ---------------------------------------------------------------------------------------------------- 2. the pass really accepts
@pytest.mark.gpu
@pytest.mark.parametrize("name,B,max_len", CASES)
def test_gpu_draft_accepts_the_common_prefix(name, B, max_len):
    m, cfg = _model(name), student_cfg(name)
    mem, ref, other_ids = _ref(name, B, max_len)
    seen = {}
    for label, d in _drafts(cfg, ref, other_ids, max_len):
        m.last_accepted = None
        m.greedy_decode(mem, max_len=max_len, stop="never", draft=d)
        assert m.last_accepted == _expected_accept(ref, d), (label, m.last_accepted)
        seen[label] = m.last_accepted
    assert seen["ref"] == max_len and seen["col 1"] == 0 and seen["col mid"] == max_len // 2 - 1
    assert seen["col last"] == max_len - 1 and seen["short"] == 3 and seen["outside the vocabulary"] == 1


# ---------------------------------------------------------------------------------------------------- 3. stop rule
# (sep bias, B, memory seed): plain greedy under all_sep stops early on the CPU oracle (checked below); found by a seed search
EARLY_STOPS = [(3.0, 1, 8), (3.0, 2, 9), (3.0, 2, 48)]


@pytest.mark.gpu
@pytest.mark.parametrize("bias,B,seed", EARLY_STOPS)
def test_gpu_draft_under_the_stop_rule(bias, B, seed):
    from gitcap.student import StudentCaptioner
    cfg, max_len = student_tiny(), 12
    w = dict(student_synthetic_weights(cfg, 0))
    w["linear.bias"] = w["linear.bias"].copy()
    w["linear.bias"][cfg.sep_token_id] += bias
    mem = make_memory(B, cfg.mem_tokens, cfg.d_model, seed)
    oracle_ids = StudentOracle(cfg, w, emulate_bf16=True).greedy_decode(mem, max_len, "all_sep")
    assert 3 <= oracle_ids.shape[1] - 1 < max_len                              # the recorded seed stops early
    m = StudentCaptioner(cfg=cfg, weights=w, device="cuda:0", max_batch=2, max_text_len=max_len)
    mem = mem.cuda()
    want = m.greedy_decode(mem, max_len=max_len, stop="all_sep").clone()
    steps = want.shape[1] - 1
    assert 3 <= steps < max_len and bool((want[:, -1] == cfg.sep_token_id).all())
    # the truncated caption as the draft: accepted whole, the stop rule fires inside the pass, no token step
    before = m._draft_stats()
    got = m.greedy_decode(mem, max_len=max_len, stop="all_sep", draft=want)
    after = m._draft_stats()
    assert torch.equal(got, want) and m.last_accepted == steps
    assert after[0] - before[0] == 1 and after[1] - before[1] == steps and after[3] - before[3] == 0
    # its last token changed: the pass corrects it (the corrected token is SEP in every row), still no token step
    d = want.clone()
    d[:, -1] = (d[:, -1] + 5) % cfg.vocab_length
    got = m.greedy_decode(mem, max_len=max_len, stop="all_sep", draft=d)
    assert torch.equal(got, want) and m.last_accepted == steps - 1
    assert m._draft_stats()[3] == after[3]
    # changed in the middle: the tail runs (a token step per remaining position) and the result stands
    d = want.clone()
    d[:, 2] = (d[:, 2] + 5) % cfg.vocab_length
    got = m.greedy_decode(mem, max_len=max_len, stop="all_sep", draft=d)
    assert torch.equal(got, want) and m.last_accepted == 1
    assert m._draft_stats()[3] - after[3] == max_len - 2
    # a draft longer than the caption (the untruncated one): same ids, same length
    full = m.greedy_decode(mem, max_len=max_len, stop="never")
    assert torch.equal(m.greedy_decode(mem, max_len=max_len, stop="all_sep", draft=full), want)


# ---------------------------------------------------------------------------------------------------- 4. the C ABI
class _Abi:
    def __init__(self, m):
        self.m, self.lib, self.h = m, m._lib, m._handle

    def err(self):
        return self.lib.gitcap_student_last_error(self.h)

    def _out(self, B, max_len):
        return (torch.full((B, max_len + 1), -1, dtype=torch.int64, device="cuda:0"),
                torch.full((1,), -1, dtype=torch.int32, device="cuda:0"))

    def greedy(self, mem, max_len, stop):
        ids, steps = self._out(mem.shape[0], max_len)
        rc = self.lib.gitcap_student_greedy(self.h, ptr(mem), mem.shape[0], max_len, stop, ptr(ids), ptr(steps), self.m._stream())
        assert rc == 0, self.err()
        return ids, steps

    def greedy_draft(self, mem, d, max_len, stop, B=None, ld=None, n=None):
        B = mem.shape[0] if B is None else B
        ids, steps = self._out(max(B, 1), max_len)
        acc = ctypes.c_int32(-7)
        rc = self.lib.gitcap_student_greedy_draft(self.h, ptr(mem), B, ptr(d), d.shape[1] if ld is None else ld,
                                                  d.shape[1] - 1 if n is None else n, max_len, stop, ptr(ids), ptr(steps),
                                                  ctypes.byref(acc), self.m._stream())
        return rc, ids, steps, acc.value

    def window_greedy(self, B, max_len, stop):
        ids, steps = self._out(B, max_len)
        rc = self.lib.gitcap_student_window_greedy(self.h, max_len, stop, ptr(ids), ptr(steps), self.m._stream())
        return rc, ids, steps

    def window_draft(self, B, d, max_len, stop, ld=None, n=None):
        ids, steps = self._out(B, max_len)
        acc = ctypes.c_int32(-7)
        rc = self.lib.gitcap_student_window_greedy_draft(self.h, ptr(d), d.shape[1] if ld is None else ld,
                                                         d.shape[1] - 1 if n is None else n, max_len, stop, ptr(ids), ptr(steps),
                                                         ctypes.byref(acc), self.m._stream())
        return rc, ids, steps, acc.value


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "base"])
def test_gpu_draft_c_abi_equals_the_plain_calls(name):
    cfg, B, max_len = student_cfg(name), 2, 10
    m = make_student(name, max_batch=4, max_text_len=12)
    a = _Abi(m)
    F = cfg.mem_tokens
    toks = make_memory(B, F + 2, cfg.d_model, 23).cuda()
    mem = toks[:, :F].contiguous()
    # plain, draft, plain: the full loop's graph is untouched and the draft call returns its result
    ids0, steps0 = a.greedy(mem, max_len, STOP_NEVER)
    d = ids0.clone()
    d[1, 4] = (d[1, 4] + 1) % cfg.vocab_length
    rc, ids1, steps1, acc = a.greedy_draft(mem, d, max_len, STOP_NEVER)
    assert rc == 0, a.err()
    assert torch.equal(ids1, ids0) and torch.equal(steps1, steps0) and acc == 3
    ids2, steps2 = a.greedy(mem, max_len, STOP_NEVER)
    assert torch.equal(ids2, ids0) and torch.equal(steps2, steps0)
    # a null accepted_out is allowed; a wide draft buffer is read by its leading dimension
    wide = torch.full((B, max_len + 4), 5, dtype=torch.int64, device="cuda:0")
    wide[:, :max_len + 1] = ids0
    ids3, steps3 = a._out(B, max_len)
    assert a.lib.gitcap_student_greedy_draft(a.h, ptr(mem), B, ptr(wide), max_len + 4, max_len, max_len, STOP_ALL_SEP, ptr(ids3),
                                             ptr(steps3), None, m._stream()) == 0, a.err()
    want_ids, want_steps = a.greedy(mem, max_len, STOP_ALL_SEP)
    n = int(want_steps.item())
    assert torch.equal(steps3, want_steps) and torch.equal(ids3[:, :1 + n], want_ids[:, :1 + n])
    # isolation: forward_decoder on fixed ids after a draft call == after the plain call
    T = 7
    y = torch.randint(1, cfg.vocab_length, (B, T), generator=torch.Generator().manual_seed(2)).cuda()
    y[:, 0] = cfg.cls_token_id

    def decoder_only():
        logits = torch.empty((B, T, cfg.vocab_length), dtype=torch.float32, device="cuda:0")
        assert a.lib.gitcap_student_forward_decoder(a.h, ptr(y), T, B, T, ptr(logits), m._stream()) == 0, a.err()
        return logits

    a.greedy(mem, max_len, STOP_NEVER)
    after_plain = decoder_only()
    assert a.greedy_draft(mem, d, max_len, STOP_NEVER)[0] == 0
    assert torch.equal(decoder_only(), after_plain)
    # the window form after six pushes, and after the ring has wrapped
    assert a.lib.gitcap_student_window_reset(a.h, B) == 0
    rc = a.window_draft(B, ids0, max_len, STOP_NEVER)[0]
    assert rc == ERR_STATE and a.err()                                          # before mem_tokens pushes
    for lo, hi in ((0, F), (F, F + 1), (F + 1, F + 2)):
        chunk = toks[:, lo:hi].contiguous()
        assert a.lib.gitcap_student_window_push(a.h, ptr(chunk), B, hi - lo, m._stream()) == 0, a.err()
        for stop in (STOP_NEVER, STOP_ALL_SEP):
            rc, want_ids, want_steps = a.window_greedy(B, max_len, stop)
            assert rc == 0, a.err()
            rc, got_ids, got_steps, acc = a.window_draft(B, ids0, max_len, stop)
            assert rc == 0, a.err()
            n = int(want_steps.item())
            assert torch.equal(got_steps, want_steps) and torch.equal(got_ids[:, :1 + n], want_ids[:, :1 + n]), (lo, stop)
            if stop == STOP_NEVER:
                assert acc == _expected_accept(want_ids, ids0)
            rc, again, _ = a.window_greedy(B, max_len, stop)
            assert rc == 0 and torch.equal(again, want_ids)
        assert torch.equal(decoder_only(), m.forward_decoder(y, toks[:, hi - F:hi].contiguous()))
    out = (ctypes.c_int64 * 4)()
    assert a.lib.gitcap_student_draft_stats(a.h, out) == 0 and out[0] == 9 and out[1] == 9 * max_len
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_draft_c_abi_errors():
    cfg, max_len = student_tiny(), 6
    m = make_student("tiny", max_batch=2, max_text_len=8)
    a = _Abi(m)
    F = cfg.mem_tokens
    mem = make_memory(2, F, cfg.d_model, 5).cuda()
    d = torch.full((2, max_len + 1), 3, dtype=torch.int64, device="cuda:0")
    ids, steps = a._out(2, max_len)
    s = m._stream()

    def refused(rc, code):
        assert rc == code, (rc, code, a.err())
        assert a.err()

    lib, h = a.lib, a.h
    assert lib.gitcap_student_greedy_draft(None, ptr(mem), 2, ptr(d), 7, 6, max_len, 0, ptr(ids), ptr(steps), None, s) == ERR_ARG
    assert lib.gitcap_student_last_error(None)                                            # a null handle: the message of the type
    refused(lib.gitcap_student_greedy_draft(h, ptr(mem), 2, None, 7, 6, max_len, 0, ptr(ids), ptr(steps), None, s), ERR_ARG)
    refused(lib.gitcap_student_greedy_draft(h, ptr(mem), 2, ptr(d), 7, 6, max_len, 0, None, ptr(steps), None, s), ERR_ARG)
    refused(lib.gitcap_student_greedy_draft(h, None, 2, ptr(d), 7, 6, max_len, 0, ptr(ids), ptr(steps), None, s), ERR_ARG)
    refused(a.greedy_draft(mem, d, max_len, STOP_NEVER, n=0)[0], ERR_ARG)
    refused(a.greedy_draft(mem, d, max_len, STOP_NEVER, n=max_len + 1, ld=max_len + 2)[0], ERR_ARG)
    refused(a.greedy_draft(mem, d, max_len, STOP_NEVER, n=6, ld=6)[0], ERR_ARG)           # ld_draft < n_draft + 1
    refused(a.greedy_draft(mem, d, 9, STOP_NEVER)[0], ERR_ARG)                            # max_len > max_text_len
    refused(a.greedy_draft(mem, d, 0, STOP_NEVER)[0], ERR_ARG)
    refused(a.greedy_draft(mem, d, max_len, 7)[0], ERR_ARG)                               # unknown stop rule
    refused(a.greedy_draft(mem, d, max_len, STOP_NEVER, B=3)[0], ERR_ARG)                 # B > max_rows
    refused(a.greedy_draft(mem, d, max_len, STOP_NEVER, B=0)[0], ERR_ARG)
    refused(lib.gitcap_student_draft_stats(h, None), ERR_ARG)
    # the window form
    refused(a.window_draft(2, d, max_len, STOP_NEVER)[0], ERR_STATE)                      # no window
    assert lib.gitcap_student_window_reset(h, 2) == 0
    refused(a.window_draft(2, d, max_len, STOP_NEVER)[0], ERR_STATE)                      # empty window
    part = mem[:, :F - 1].contiguous()
    assert lib.gitcap_student_window_push(h, ptr(part), 2, F - 1, s) == 0
    refused(a.window_draft(2, d, max_len, STOP_NEVER)[0], ERR_STATE)                      # F - 1 tokens
    refused(lib.gitcap_student_window_push(h, ptr(part), 1, 1, s), ERR_ARG)                # B different from the reset's
    last = mem[:, F - 1:].contiguous()
    assert lib.gitcap_student_window_push(h, ptr(last), 2, 1, s) == 0
    rc, got, _, acc = a.window_draft(2, d, max_len, STOP_NEVER)
    assert rc == 0 and torch.equal(got, a.greedy(mem, max_len, STOP_NEVER)[0]) and 0 <= acc <= max_len
    assert lib.gitcap_student_window_greedy_draft(None, ptr(d), 7, 6, max_len, 0, ptr(ids), ptr(steps), None, s) == ERR_ARG
    refused(lib.gitcap_student_window_greedy_draft(h, None, 7, 6, max_len, 0, ptr(ids), ptr(steps), None, s), ERR_ARG)
    refused(lib.gitcap_student_window_greedy_draft(h, ptr(d), 7, 6, max_len, 0, None, ptr(steps), None, s), ERR_ARG)
    refused(a.window_draft(2, d, max_len, STOP_NEVER, n=0)[0], ERR_ARG)
    refused(a.window_draft(2, d, max_len, STOP_NEVER, n=7, ld=8)[0], ERR_ARG)
    refused(a.window_draft(2, d, max_len, STOP_NEVER, n=6, ld=6)[0], ERR_ARG)
    refused(a.window_draft(2, d, 9, STOP_NEVER)[0], ERR_ARG)
    refused(a.window_draft(2, d, max_len, 7)[0], ERR_ARG)
    torch.cuda.synchronize()
    # weights not finalized
    from gitcap.student import StudentCaptioner
    raw = _Abi(StudentCaptioner(cfg=cfg, device="cuda:0", max_batch=2, max_text_len=8))
    assert raw.greedy_draft(mem, d, max_len, STOP_NEVER)[0] == ERR_STATE and raw.err()
    assert raw.window_draft(2, d, max_len, STOP_NEVER)[0] == ERR_STATE


_NO_GRAPH_CHILD = r"""
import sys
sys.path[:0] = [%r, %r]
import torch
from gitcap.student import StudentCaptioner
from gitcap.student_config import student_synthetic_weights, student_tiny
from oracle.student_oracle import make_memory
cfg = student_tiny()
m = StudentCaptioner(cfg=cfg, weights=student_synthetic_weights(cfg, 0), device="cuda:0", max_batch=2, max_text_len=12)
for B in (1, 2):
    mem = make_memory(B, cfg.mem_tokens, cfg.d_model, 40 + B).cuda()
    ref = m.greedy_decode(mem, max_len=12, stop="never").clone()
    for c in (None, 1, 6, 12):
        d = ref.clone()
        if c is not None:
            d[:, c] = (d[:, c] + 1) %% cfg.vocab_length
        assert torch.equal(m.greedy_decode(mem, max_len=12, stop="never", draft=d), ref), (B, c)
        assert m.last_accepted == (12 if c is None else c - 1), (B, c, m.last_accepted)
        assert torch.equal(m.greedy_decode(mem, max_len=12, stop="never"), ref), (B, c)
    print("ids", B, ref.tolist())
print("child ok")
"""


@pytest.mark.gpu
def test_gpu_draft_without_graphs_in_a_fresh_process():
    """GITCAP_STUDENT_GRAPH=0 is read once per process: plain, draft, plain launched kernel by kernel give the graphs' ids."""
    env = dict(os.environ, GITCAP_STUDENT_GRAPH="0")
    code = _NO_GRAPH_CHILD % (ROOT, os.path.join(ROOT, "real-time-video-captioning_amd"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr
    m, cfg = _model("tiny"), student_tiny()
    for B in (1, 2):
        mem = make_memory(B, cfg.mem_tokens, cfg.d_model, 40 + B).cuda()
        assert f"ids {B} {m.greedy_decode(mem, max_len=12, stop='never').tolist()}" in r.stdout


# ---------------------------------------------------------------------------------------------------- 5. the stream
@pytest.mark.gpu
@pytest.mark.parametrize("batch", [1, 2])
def test_gpu_caption_stream_carries_its_caption(batch):
    max_len = 12
    ma = make_student_native("tiny", tinyvit="tiny", max_batch=4, max_text_len=16)
    mb = make_student_native("tiny", tinyvit="tiny", max_batch=4, max_text_len=16)
    F = ma.cfg.mem_tokens
    cam = torch.randint(0, 256, (batch, 14, 64, 80, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(31 + batch))
    cam[:, 6:12] = cam[:, 6:7]                                                  # frames 6..11: one repeated frame
    cam = cam.cuda()
    with pytest.raises(ValueError):
        ma.caption_stream(batch=batch, hop=1, max_len=max_len, beams=3, carry=True)
    sa = ma.caption_stream(batch=batch, hop=1, max_len=max_len, stop="never", carry=True)
    sb = mb.caption_stream(batch=batch, hop=1, max_len=max_len, stop="never")
    captions, prev = 0, None
    for i in range(14):
        got, want = sa.push(cam[:, i]), sb.push(cam[:, i])
        if i < F - 1:
            assert got is None and want is None
            continue
        captions += 1
        assert torch.equal(got, want), i
        last = sa.stats()["last"]
        if prev is None:
            assert last == dict(draft_tokens=0, accepted=0, tail_steps=0)      # the first caption: the plain call
        else:
            acc = _expected_accept(want, prev)
            assert last == dict(draft_tokens=max_len, accepted=acc, tail_steps=max(max_len - 1 - acc, 0)), (i, last)
        prev = want
    st = sa.stats()
    assert st["captions"] == captions == 9 and st["draft_tokens"] == 8 * max_len
    assert sb.stats()["draft_tokens"] == 0 and sb.stats()["captions"] == 9
    # the repeated frame until two windows in a row hold nothing else: the second one's draft is its own caption
    for i in range(F + 1):
        got, want = sa.push(cam[:, 6]), sb.push(cam[:, 6])
        assert torch.equal(got, want), i
    assert sa.stats()["last"] == dict(draft_tokens=max_len, accepted=max_len, tail_steps=0)
    # reset(): the next caption is a plain call again, and the one after it carries
    sa.reset()
    sb.reset()
    for i in range(F):
        got, want = sa.push(cam[:, i]), sb.push(cam[:, i])
    assert torch.equal(got, want) and sa.stats()["last"]["draft_tokens"] == 0
    got, want = sa.push(cam[:, F]), sb.push(cam[:, F])
    assert torch.equal(got, want) and sa.stats()["last"]["draft_tokens"] == max_len


# ---------------------------------------------------------------------------------------------------- 6. speed switches
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["tiny", "base"])
def test_gpu_draft_speed_switches_change_nothing(name):
    """Keys 1 (row prologue) and 10 (shared-row vocabulary head) are speed-only on the draft path too; the token-step graphs are
    captured again per switch setting."""
    from gitcap import _lib
    lib = _lib.load()
    m, cfg = _model(name), student_cfg(name)
    mem, ref, other_ids = _ref(name, 1, 25)
    drafts = _drafts(cfg, ref, other_ids, 25)
    for key in (1, 10):
        old = lib.gitcap_dbg_config(key, 0)
        try:
            for label, d in drafts:
                assert torch.equal(m.greedy_decode(mem, max_len=25, stop="never", draft=d), ref), (key, label)
                assert m.last_accepted == _expected_accept(ref, d), (key, label)
        finally:
            lib.gitcap_dbg_config(key, old)
    for label, d in drafts:
        assert torch.equal(m.greedy_decode(mem, max_len=25, stop="never", draft=d), ref), label
