"""The student's constrained decoding end to end on the tiny model (V = 97), through the public surface: the device loops under
no_repeat_ngram_size / min_length / suppress_tokens against a host loop of forward_decoder on the growing prefix -> the restatement's
mask -> first arg-max (exact ids: a cached step is bit for bit the teacher-forced position), the streams and the pool against
greedy_decode under the same rules, the beam search against beam_search_host, and the attachment's life cycle at the C level."""
import ctypes
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import logprob_reference as LPR
import student_constraints_support as S
from gitcap import _lib
from gitcap.student import StudentCaptioner
from gitcap.student_config import student_synthetic_weights, student_tiny
from gpu_support import camera, ptr, same_bits, stream, tinyvit_cfg
from oracle.student_oracle import make_memory

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
B, L, K = S.B, S.L, S.K
TOL = 2e-5                          # tests/test_logprob_gpu.py derives it
KW = dict(device="cuda:0", max_batch=9, max_text_len=12, stop="never")


def _bites(got, unconstrained, kw, sep):
    """Where a row of the unconstrained result breaks the rules the constrained result must differ -> whether that is so here"""
    broken = not all(S.obeys(r, kw, sep) for r in unconstrained.cpu())
    assert not (broken and torch.equal(got.cpu(), unconstrained.cpu())), kw
    return broken


def _with_early_sep(build):
    """build(cfg) -> (model, free caption ids); SEP becomes a token the free caption emits early, so that min_length bites"""
    cfg = student_tiny()
    _, free = build(cfg)
    cfg = dataclasses.replace(cfg, sep_token_id=int(free[0, 2]))
    m, free = build(cfg)
    return m, cfg, free.clone()


@pytest.fixture(scope="module")
def model():
    assert torch.cuda.is_available()
    w = student_synthetic_weights(student_tiny(), 0)
    mem = make_memory(B, student_tiny().mem_tokens, student_tiny().d_model, S.MEM_SEED).cuda()

    def build(cfg):
        m = StudentCaptioner(cfg=cfg, weights=w, **KW)
        return m, m.greedy_decode(mem, max_len=L)
    m, cfg, free = _with_early_sep(build)
    return m, cfg, mem, free


@pytest.fixture(scope="module")
def host_loops(model):
    """case index -> (ids [B][1 + L], the masked rows [L][B][V]) of the host loop, computed once"""
    m, cfg, mem, free = model
    out = {}
    for i, case in enumerate(S.CASES):
        out[i] = S.greedy_yardstick(lambda ids, me: m.forward_decoder(ids.cuda(), me), mem, L, S.case_kw(case, free), cfg.cls_token_id,
                                    cfg.sep_token_id, cfg.vocab_length)
    return out


@pytest.mark.parametrize("i", range(len(S.CASES)))
@pytest.mark.parametrize("stop", ["never", "all_sep"])
def test_greedy_equals_the_host_loop(model, host_loops, i, stop):
    m, cfg, mem, free = model
    kw = S.case_kw(S.CASES[i], free)
    want, rows = host_loops[i]
    got = m.greedy_decode(mem, max_len=L, stop=stop, **kw)
    n = got.shape[1] - 1
    assert (n == L or stop == "all_sep") and n >= 1
    assert torch.equal(got.cpu(), want[:, :1 + n]), (got, want)
    assert not torch.equal(got, free[:, :1 + n])                # the case bites
    for b in range(B):                                          # each row alone
        one = m.greedy_decode(mem[b:b + 1], max_len=L, stop="never", **kw)
        assert torch.equal(one[:, :1 + n], got[b:b + 1]), b
    ids2, lp, top_ids, top_lp = m.greedy_decode(mem, max_len=L, stop=stop, return_logprobs=True, top_logprobs=4, **kw)
    assert torch.equal(ids2, got)
    want_lp = np.stack([LPR.token_logprobs(rows[t])[1] for t in range(n)], 1)
    err = np.abs(lp.cpu().numpy().astype(np.float64) - want_lp).max()
    print(f"{kw} stop={stop}: max |log-probability - restatement over the masked row| {err:.3e}")
    assert err <= TOL
    assert torch.equal(top_ids[:, :, 0], got[:, 1:]) and bool((top_lp[:, :, 0] == lp).all())
    tid = top_ids.cpu().numpy()
    nbanned = 0
    for t in range(n):
        for b in range(B):
            banned = set(np.nonzero(np.isinf(rows[t][b]))[0].tolist())      # (may be empty: a 2-gram rule behind min_length)
            nbanned += len(banned)
            assert not banned & set(tid[b, t].tolist()), (t, b)
    assert nbanned > 0
    assert torch.equal(m.greedy_decode(mem, max_len=L, stop="never"), free)      # the next call without keywords is the free caption
    for b in range(B):
        assert S.obeys(got[b].cpu(), kw, cfg.sep_token_id), (kw, got[b])


def test_one_graph_serves_different_rules_back_to_back(model, host_loops):
    m, cfg, mem, free = model
    for i in (0, 3, 1, 3, 2, 0):
        got = m.greedy_decode(mem, max_len=L, **S.case_kw(S.CASES[i], free))
        assert torch.equal(got.cpu(), host_loops[i][0]), i
    assert torch.equal(m.greedy_decode(mem, max_len=L), free)


_NO_GRAPH_CHILD = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import dataclasses
import torch
import student_constraints_support as S
from gitcap.student import StudentCaptioner
from gitcap.student_config import student_synthetic_weights, student_tiny
from oracle.student_oracle import make_memory
cfg = dataclasses.replace(student_tiny(), sep_token_id=%d)
m = StudentCaptioner(cfg=cfg, weights=student_synthetic_weights(student_tiny(), 0), device="cuda:0", max_batch=9, max_text_len=12, stop="never")
mem = make_memory(S.B, cfg.mem_tokens, cfg.d_model, S.MEM_SEED).cuda()
free = m.greedy_decode(mem, max_len=S.L).clone()
print("free", free.tolist())
for i, case in enumerate(S.CASES):
    print("case", i, m.greedy_decode(mem, max_len=S.L, **S.case_kw(case, free)).tolist())
    assert torch.equal(m.greedy_decode(mem, max_len=S.L), free)
print("child ok")
"""


def test_same_ids_without_graphs_in_a_fresh_process(model, host_loops):
    """GITCAP_STUDENT_GRAPH=0 is read once per process: the same launches kernel by kernel give the graphs' ids."""
    m, cfg, mem, free = model
    env = dict(os.environ, GITCAP_STUDENT_GRAPH="0")
    code = _NO_GRAPH_CHILD % (ROOT, os.path.join(ROOT, "real-time-video-captioning_amd"), os.path.join(ROOT, "tests"), cfg.sep_token_id)
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr
    assert f"free {free.tolist()}" in r.stdout
    for i in range(len(S.CASES)):
        assert f"case {i} {host_loops[i][0].tolist()}" in r.stdout, i


@pytest.mark.parametrize("i", [1, 3])
def test_ragged_clips_equal_the_clips_alone(model, i):
    m, cfg, mem, free = model
    kw = S.case_kw(S.CASES[i], free)
    F = cfg.mem_tokens
    clips = [mem[0, :F], mem[1, :2], mem[2, :1]]              # (clip 0 is the full clip whose free caption holds SEP early)
    got = m.greedy_decode(clips, max_len=L, **kw)
    unc = m.greedy_decode(clips, max_len=L)
    assert _bites(got, unc, kw, cfg.sep_token_id)
    for b, c in enumerate(clips):
        assert torch.equal(m.greedy_decode([c], max_len=L, **kw), got[b:b + 1]), b
        assert S.obeys(got[b].cpu(), kw, cfg.sep_token_id)
    assert torch.equal(m.greedy_decode(clips, max_len=L), unc)


# ---- the live paths (native encoder) --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def native():
    from gitcap.tinyvit import TinyViTEncoder
    from gitcap.tinyvit_config import tinyvit_synthetic_weights
    tcfg = tinyvit_cfg("tiny")
    weights = dict(student_synthetic_weights(student_tiny(), 0))
    weights.update({"image_encoder.model." + k: v for k, v in tinyvit_synthetic_weights(tcfg, 0).items()})
    s, F = tcfg.img_size, student_tiny().mem_tokens
    cams = camera((B, F + 2, s, s, 3), 171)

    def build(cfg):
        enc = TinyViTEncoder(tcfg, device="cuda:0", max_frames=9 * cfg.mem_tokens)
        m = StudentCaptioner(cfg=cfg, weights=weights, image_encoder=enc, device="cuda:0", max_batch=9, max_text_len=12)
        return m, m.greedy_decode(cams[:, :F], max_len=L, stop="never")
    m, cfg, free = _with_early_sep(build)
    return m, cfg, cams, free


def _eq(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert torch.equal(a, b) if a.dtype == torch.int64 else same_bits(a.contiguous(), b.contiguous()), what


@pytest.mark.parametrize("i", [1, 3])
@pytest.mark.parametrize("partial", [False, True])
def test_caption_stream_equals_greedy_decode_under_the_same_rules(native, i, partial):
    m, cfg, cams, free = native
    kw = S.case_kw(S.CASES[i], free)
    F = cfg.mem_tokens
    st = m.caption_stream(batch=B, hop=1, max_len=L, stop="never", logprobs=True, partial=partial, **kw)
    captions = 0
    for j in range(F + 2):
        out = st.push(cams[:, j])
        n = min(j + 1, F)
        if n < F and not partial:
            assert out is None
            continue
        win = cams[:, j + 1 - n:j + 1]
        ref, ref_lp = m.greedy_decode(win if n == F else [win[b] for b in range(B)], max_len=L, stop="never", return_logprobs=True, **kw)
        _eq(out, ref, f"push {j + 1}")
        _eq(st.last_logprobs, ref_lp, f"logprobs of push {j + 1}")
        assert st.last_frames == n
        for b in range(B):
            assert S.obeys(out[b], kw, cfg.sep_token_id)
        bit = _bites(out, m.greedy_decode(win if n == F else [win[b] for b in range(B)], max_len=L, stop="never"), kw, cfg.sep_token_id)
        assert bit or j != F - 1                            # the first full window: its free caption holds SEP early
        captions += 1
    assert captions == (F + 2 if partial else 3)
    with pytest.raises(ValueError, match="carry=True is not combined"):
        m.caption_stream(batch=1, carry=True, max_len=L, **kw)


@pytest.mark.parametrize("i", [1, 3])
def test_stream_pool_equals_greedy_decode_under_the_same_rules(native, i):
    m, cfg, cams, free = native
    kw = S.case_kw(S.CASES[i], free)
    F, sep = cfg.mem_tokens, cfg.sep_token_id
    pool = m.stream_pool(B, hop=1, max_len=L, logprobs=True, **kw)           # the model's stop rule: all_sep, cut per row
    pushes = [[0], [2, 0, 1], [1, 1], [0, 1, 2], [2, 2, 0, 1], [1, 2, 1], [0, 0, 2]]
    at = [0] * B
    differs = False
    for p in pushes:
        frames = []
        for c in p:
            frames.append(cams[c, at[c]])
            at[c] += 1
        out = pool.push(torch.stack(frames, 0), p)
        assert sorted(out) == sorted(set(p))
        for c, ids in out.items():
            n = min(at[c], F)
            clip = [cams[c, at[c] - n:at[c]]]
            ref, ref_lp = m.greedy_decode(clip, max_len=L, stop="never", return_logprobs=True, **kw)
            hits = (ref[0, 1:] == sep).nonzero()
            k = int(hits[0]) + 1 if hits.numel() else L
            _eq(ids, ref[0, :1 + k], f"camera {c} after {at[c]} frames")
            _eq(pool.last_logprobs[c], ref_lp[0, :k], f"logprobs of camera {c} after {at[c]} frames")
            assert S.obeys(ref[0], kw, sep)
            differs |= not torch.equal(ref, m.greedy_decode(clip, max_len=L, stop="never"))
    assert differs and max(at) > F


# ---- beam search ---------------------------------------------------------------------------------------------------------------------

def test_beam_search_equals_the_host_search_under_the_same_rules(model, golden_dir):
    m, cfg, _, free = model
    g = np.load(os.path.join(golden_dir, "student_tiny.npz"))
    mem = make_memory(3, cfg.mem_tokens, cfg.d_model, int(g["mem_seed"])).cuda()
    base = m.beam_search(mem, max_len=9, k=K)
    assert torch.equal(base, m.beam_search_host(mem, max_len=9, k=K))
    own = sorted({int(v) for v in base[:, 1:3].reshape(-1).tolist()})
    bites = 0
    for kw in (dict(no_repeat_ngram_size=1), dict(no_repeat_ngram_size=2, min_length=6), dict(min_length=10),
               dict(no_repeat_ngram_size=3, min_length=4, suppress_tokens=own)):
        dev = m.beam_search(mem, max_len=9, k=K, **kw)
        assert torch.equal(dev, m.beam_search_host(mem, max_len=9, k=K, **kw)), kw
        for b in range(3):
            assert S.obeys(dev[b].cpu(), kw, cfg.sep_token_id), (kw, dev[b])
        clips = [mem[0, :2], mem[1], mem[2, :3]]                                # ragged: every clip is the clip alone
        rag = m.beam_search(clips, max_len=9, k=K, **kw)
        for b, c in enumerate(clips):
            assert torch.equal(m.beam_search([c], max_len=9, k=K, **kw), rag[b:b + 1]), (kw, b)
        bites += _bites(dev, base, kw, cfg.sep_token_id)
    assert bites >= 1 and not torch.equal(dev, base)        # (the last case suppresses the free beams' own tokens)
    assert torch.equal(m.beam_search(mem, max_len=9, k=K), base)
    with pytest.raises(ValueError):
        m.beam_search(mem, max_len=9, k=K, suppress_tokens=list(range(cfg.vocab_length - 9 - K + 1)))


def test_caption_stream_beams_equal_the_host_search(native):
    m, cfg, cams, free = native
    F = cfg.mem_tokens
    kw = dict(no_repeat_ngram_size=2, min_length=6, suppress_tokens=[int(free[0, 1]), int(free[1, 1])])
    st = m.caption_stream(batch=B, hop=1, max_len=9, beams=K, **kw)
    out = None
    for j in range(F + 1):
        out = st.push(cams[:, j])
        assert (out is None) == (j + 1 < F)
        if out is not None:
            win = cams[:, j + 1 - F:j + 1]
            assert torch.equal(out, m.beam_search_host(win, max_len=9, k=K, **kw)), j
            assert torch.equal(out, m.beam_search(win, max_len=9, k=K, **kw)), j
            _bites(out, m.beam_search(win, max_len=9, k=K), kw, cfg.sep_token_id)
            for b in range(B):
                assert S.obeys(out[b].cpu(), kw, cfg.sep_token_id)


# ---- refusals and the life cycle -------------------------------------------------------------------------------------------------------

def test_life_cycle_and_refusals(model):
    m, cfg, mem, free = model
    lib, h, V = m._lib, m._handle, cfg.vocab_length
    ids = torch.zeros((B, L + 1), dtype=torch.int64, device="cuda")
    steps = torch.zeros((1,), dtype=torch.int32, device="cuda")
    acc = ctypes.c_int32(-1)
    sup = torch.tensor([int(free[0, 1]), int(free[1, 1]), int(free[2, 1])], dtype=torch.int32, device="cuda")
    c = _lib.CConstraints(1, 0, sup.data_ptr(), 3)
    logits = torch.empty((B, 1, V), device="cuda")

    def greedy(max_len=L):
        rc = lib.gitcap_student_greedy(h, ptr(mem), B, max_len, 0, ptr(ids), ptr(steps), stream())
        torch.cuda.synchronize()
        return rc

    def attach(cc=c):
        return lib.gitcap_student_attach_constraints(h, ctypes.byref(cc) if cc is not None else None)
    assert attach() == 0 and attach(None) == 0
    assert attach() == 0
    # set_memory and forward_decoder leave it pending
    assert lib.gitcap_student_set_memory(h, ptr(mem), B, stream()) == 0
    assert lib.gitcap_student_forward_decoder(h, ptr(free[:, :1].contiguous()), 1, B, 1, ptr(logits), stream()) == 0
    assert greedy() == 0 and not torch.equal(ids, free)
    constrained = ids.clone()
    assert greedy() == 0 and torch.equal(ids, free)         # consumed: the next call is unconstrained
    assert attach() == 0 and greedy(max_len=99) == ERR_ARG  # a refused call consumes it
    assert greedy() == 0 and torch.equal(ids, free)
    assert attach() == 0 and attach(None) == 0              # NULL detaches
    assert greedy() == 0 and torch.equal(ids, free)
    # a draft call consumes it and refuses
    assert attach() == 0
    rc = lib.gitcap_student_greedy_draft(h, ptr(mem), B, ptr(free), L + 1, L, L, 0, ptr(ids), ptr(steps), ctypes.byref(acc), stream())
    assert rc == ERR_ARG and b"constraints" in lib.gitcap_student_last_error(h)
    assert greedy() == 0 and torch.equal(ids, free)
    for bad in (_lib.CConstraints(-1, 0, None, 0), _lib.CConstraints(0, -1, None, 0), _lib.CConstraints(0, 0, None, -1),
                _lib.CConstraints(0, 0, sup.data_ptr(), 257), _lib.CConstraints(0, 0, None, 2), _lib.CConstraints(0, 0, sup.data_ptr() + 2, 2)):
        assert attach(bad) == ERR_ARG
    assert greedy() == 0 and torch.equal(ids, free)         # nothing was left attached; the handle is usable
    # n_suppress + max_len >= V: refused at the consuming call, and the call behind it is unconstrained
    many = torch.arange(V - L, dtype=torch.int32, device="cuda")
    assert many.numel() <= 256 and many.numel() + L >= V
    assert attach(_lib.CConstraints(0, 0, many.data_ptr(), many.numel())) == 0
    assert greedy() == ERR_ARG
    assert greedy() == 0 and torch.equal(ids, free)
    best = torch.zeros((1, 9), dtype=torch.int64, device="cuda")
    fits = many[:V - 9 - K + 1]                              # n_suppress + max_len + k == V + 1: one too many for the beam family
    assert attach(_lib.CConstraints(0, 0, fits.data_ptr(), fits.numel())) == 0
    assert lib.gitcap_student_beam_search(h, ptr(mem), 1, K, 9, ptr(best), stream()) == ERR_ARG
    assert attach(_lib.CConstraints(0, 0, fits.data_ptr(), fits.numel() - 1)) == 0
    assert lib.gitcap_student_beam_search(h, ptr(mem), 1, K, 9, ptr(best), stream()) == 0
    torch.cuda.synchronize()
    assert not set(best[0, 1:].tolist()) & set(fits[:-1].tolist())
    with pytest.raises(ValueError, match="draft= is not combined"):
        m.greedy_decode(mem, max_len=L, draft=free, no_repeat_ngram_size=2)
    with pytest.raises(ValueError):
        m.greedy_decode(mem, max_len=L, no_repeat_ngram_size=-1)
    with pytest.raises(ValueError):
        m.greedy_decode(mem, max_len=L, suppress_tokens=list(range(257)))
    with pytest.raises(ValueError):
        m.greedy_decode(mem, max_len=L, suppress_tokens=list(range(V - L)))
    assert attach() == 0
    assert greedy() == 0 and torch.equal(ids, constrained)
    assert torch.equal(m.greedy_decode(mem, max_len=L), free)
