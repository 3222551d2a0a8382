"""The student's prompted decoding end to end on the tiny model (V = 97, B = 3, max_len 10, k = 3), through the public surface and
exact: the device loops against a host loop of forward_decoder on the growing prefix that takes the prompt's token inside a row's
prompt (a cached step is bit for bit the teacher-forced position), the one-pass plan against forced steps, log-probabilities,
constraints and alternatives at forced positions, ragged memories, the stream and the pool against greedy_decode, the beam search
against beam_search_host, and the attachment's life cycle at the C level."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import student_constraints_support as S
import student_prompt_reference as P
from gitcap.student import StudentCaptioner
from gitcap.student_config import student_synthetic_weights, student_tiny
from gpu_support import camera, ptr, same_bits, stream, tinyvit_cfg
from oracle.student_oracle import make_memory

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG = -1
B, L, K = P.B, P.L, P.K
KW = dict(device="cuda:0", max_batch=9, max_text_len=12, stop="never")


def _rows(prompts):
    return [torch.tensor(r, dtype=torch.int64) for r in prompts]


@pytest.fixture(scope="module")
def model():
    assert torch.cuda.is_available()
    cfg = student_tiny()
    m = StudentCaptioner(cfg=cfg, weights=student_synthetic_weights(cfg, 0), **KW)
    mem = make_memory(B, cfg.mem_tokens, cfg.d_model, P.MEM_SEED).cuda()
    free = m.greedy_decode(mem, max_len=L).clone()
    return m, cfg, mem, free


@pytest.fixture(scope="module")
def cases(model):
    """case -> (prompts, the host loop's (ids, forced, logits)), computed once"""
    m, cfg, mem, free = model
    out = {}
    for name, prompts in P.case_prompts(free.cpu().numpy(), cfg.vocab_length, cfg.cls_token_id).items():
        out[name] = (prompts, P.greedy_yardstick(lambda ids, me: m.forward_decoder(ids.cuda(), me), mem, L, prompts, cfg.cls_token_id))
    return out


@pytest.mark.parametrize("name", ["shared4", "ragged"])
def test_greedy_equals_the_host_loop(model, cases, name):
    m, cfg, mem, free = model
    prompts, (want, forced, _) = cases[name]
    got = m.greedy_decode(mem, max_len=L, prompt=_rows(prompts))
    assert np.array_equal(got.cpu().numpy(), want), (got, want)
    for b, row in enumerate(prompts):                              # the case bites: behind a prompt the model emits other tokens
        n = len(row)
        assert got[b, :n].tolist() == row
        assert torch.equal(got[b], free[b]) if n == 1 else bool((got[b, n:] != free[b, n:]).any()), (name, b)
        one = m.greedy_decode(mem[b:b + 1], max_len=L, prompt=[torch.tensor(row)])
        assert torch.equal(one, got[b:b + 1]), b                    # each row alone
    ids, lens = P.table(prompts, cfg.cls_token_id)                  # the [B, P] + prompt_lengths form, CLS left out of the tensor
    assert torch.equal(m.greedy_decode(mem, max_len=L, prompt=torch.as_tensor(ids), prompt_lengths=torch.as_tensor(lens)), got)
    cut = m.greedy_decode(mem, max_len=L, stop="all_sep", prompt=_rows(prompts))
    assert cut.shape[1] >= 2 and torch.equal(cut, got[:, :cut.shape[1]])
    assert torch.equal(m.greedy_decode(mem, max_len=L), free)       # the call behind a prompted call is the call made before it


def test_one_pass_equals_forced_steps(model, cases):
    """Row b of the shared 4-token prompt runs as one pass in its own batch (min_len 4) and as forced token steps beside a row
    without a prompt (min_len 1); so does the whole batch with the one-pass plan switched off."""
    m, cfg, mem, free = model
    prompts, (want, _, _) = cases["shared4"]
    cls = [cfg.cls_token_id]
    for b in range(B):
        o = (b + 1) % B
        pair = m.greedy_decode(torch.stack([mem[b], mem[o]]), max_len=L, prompt=_rows([prompts[b], cls]))
        assert pair[0].tolist() == want[b].tolist() and torch.equal(pair[1], free[o]), b
    old = m._lib.gitcap_dbg_config(20, 0)
    try:
        steps, steps_lp = m.greedy_decode(mem, max_len=L, prompt=_rows(prompts), return_logprobs=True)
    finally:
        m._lib.gitcap_dbg_config(20, old)
    one, one_lp = m.greedy_decode(mem, max_len=L, prompt=_rows(prompts), return_logprobs=True)
    assert np.array_equal(steps.cpu().numpy(), want) and torch.equal(one, steps) and same_bits(one_lp, steps_lp)
    full = [free[b, :L].tolist() for b in range(B)]                 # min_len == max_len: one pass, then the single free position
    assert torch.equal(m.greedy_decode(mem, max_len=L, prompt=_rows(full)), free)


@pytest.mark.parametrize("name", ["shared4", "ragged"])
def test_logprobs_are_zero_inside_a_prompt_and_the_scores_behind_it(model, cases, name):
    m, cfg, mem, free = model
    prompts, (want, forced, _) = cases[name]
    ids, lp = m.greedy_decode(mem, max_len=L, prompt=_rows(prompts), return_logprobs=True)
    assert np.array_equal(ids.cpu().numpy(), want)
    sc = m.score(mem, ids, until_sep=False)["token_logprobs"]
    f = torch.as_tensor(forced).cuda()
    assert bool((lp[f] == 0.0).all()) and f.any() and bool((lp[~f] == sc[~f]).all()) and bool((lp[~f] < 0).all())


def test_constraints_and_alternatives_at_forced_positions(model, cases):
    m, cfg, mem, free = model
    prompts, (want, forced, logits) = cases["ragged"]
    banned = sorted({prompts[1][1], prompts[2][4], int(want[0, 2])})          # two prompt tokens and one the model emits freely
    kw = dict(no_repeat_ngram_size=2, suppress_tokens=banned)
    ids, lp, top_ids, top_lp = m.greedy_decode(mem, max_len=L, prompt=_rows(prompts), return_logprobs=True, top_logprobs=4, **kw)
    unc = m.greedy_decode(mem, max_len=L, prompt=_rows(prompts))
    assert not torch.equal(ids, unc)
    f = torch.as_tensor(forced).cuda()
    for b, row in enumerate(prompts):
        n = len(row)
        assert ids[b, :n].tolist() == row                           # emitted although banned
        assert not set(ids[b, n:].tolist()) & set(banned)           # the rules hold behind the prompt
        assert S.obeys(ids[b, n - 1:].cpu(), dict(kw, suppress_tokens=[]) if n > 1 else kw, cfg.sep_token_id), (b, ids[b])
        seq = ids[b].tolist()
        grams = [tuple(seq[i:i + 2]) for i in range(len(seq) - 1)]
        assert all(grams.index(g) == i or i + 1 < n for i, g in enumerate(grams)), (b, seq)   # a repeated 2-gram ends inside the prompt only
    assert prompts[1][1] in ids[1].tolist() and prompts[2][4] in ids[2].tolist()
    assert bool((lp[f] == 0.0).all())
    # ranks at a forced position are the model's own: rank 0 is the masked row's arg-max, not the prompt's token
    assert bool((top_ids[~f][:, 0] == ids[:, 1:][~f]).all()) and bool((top_lp[~f][:, 0] == lp[~f]).all())
    assert bool(torch.isfinite(top_lp[f]).all()) and bool((top_lp[f][:, 0] >= top_lp[f][:, 1]).all())
    assert bool((top_ids[f][:, 0] != ids[:, 1:][f]).any())
    plain_ids, plain_top, _ = m.greedy_decode(mem, max_len=L, prompt=_rows(prompts), top_logprobs=4)
    assert torch.equal(plain_ids, unc)
    am = torch.as_tensor(logits.argmax(-1).T).cuda()                # the host loop's arg-max of every step [B][L]
    assert torch.equal(plain_top[:, :, 0], am)


def test_ragged_memory_with_a_prompt_equals_the_clip_alone(model, cases):
    m, cfg, mem, free = model
    prompts, _ = cases["ragged"]
    pr = [prompts[2], prompts[0], prompts[1]]
    clips = [mem[0], mem[1, :2], mem[2, :1]]
    got = m.greedy_decode(clips, max_len=L, prompt=_rows(pr))
    for b, c in enumerate(clips):
        assert torch.equal(m.greedy_decode([c], max_len=L, prompt=_rows(pr[b:b + 1])), got[b:b + 1]), b
        assert got[b, :len(pr[b])].tolist() == pr[b]
    assert not torch.equal(got, m.greedy_decode(clips, max_len=L))


_NO_GRAPH_CHILD = r"""
import sys
sys.path[:0] = [%r, %r, %r]
import torch
import student_prompt_reference as P
from gitcap.student import StudentCaptioner
from gitcap.student_config import student_synthetic_weights, student_tiny
from oracle.student_oracle import make_memory
cfg = student_tiny()
m = StudentCaptioner(cfg=cfg, weights=student_synthetic_weights(cfg, 0), device="cuda:0", max_batch=9, max_text_len=12, stop="never")
mem = make_memory(P.B, cfg.mem_tokens, cfg.d_model, P.MEM_SEED).cuda()
free = m.greedy_decode(mem, max_len=P.L).clone()
print("free", free.tolist())
for name, prompts in P.case_prompts(free.cpu().numpy(), cfg.vocab_length, cfg.cls_token_id).items():
    print("case", name, m.greedy_decode(mem, max_len=P.L, prompt=[torch.tensor(r) for r in prompts]).tolist())
    assert torch.equal(m.greedy_decode(mem, max_len=P.L), free)
print("child ok")
"""


def test_same_ids_without_graphs_in_a_fresh_process(model, cases):
    """GITCAP_STUDENT_GRAPH=0 is read once per process: the same launches kernel by kernel give the graphs' ids."""
    m, cfg, mem, free = model
    env = dict(os.environ, GITCAP_STUDENT_GRAPH="0")
    code = _NO_GRAPH_CHILD % (ROOT, os.path.join(ROOT, "real-time-video-captioning_amd"), os.path.join(ROOT, "tests"))
    r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr
    assert f"free {free.tolist()}" in r.stdout
    for name, (_, (want, _, _)) in cases.items():
        assert f"case {name} {want.tolist()}" in r.stdout, name


# ---- the live paths (native encoder) --------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def native():
    from gitcap.tinyvit import TinyViTEncoder
    from gitcap.tinyvit_config import tinyvit_synthetic_weights
    tcfg = tinyvit_cfg("tiny")
    cfg = student_tiny()
    weights = dict(student_synthetic_weights(cfg, 0))
    weights.update({"image_encoder.model." + k: v for k, v in tinyvit_synthetic_weights(tcfg, 0).items()})
    s, F = tcfg.img_size, cfg.mem_tokens
    cams = camera((B, F + 2, s, s, 3), 171)
    enc = TinyViTEncoder(tcfg, device="cuda:0", max_frames=9 * cfg.mem_tokens)
    m = StudentCaptioner(cfg=cfg, weights=weights, image_encoder=enc, device="cuda:0", max_batch=9, max_text_len=12)
    free = m.greedy_decode(cams[:, :F], max_len=L, stop="never")
    return m, cfg, cams, free, P.case_prompts(free.cpu().numpy(), cfg.vocab_length, cfg.cls_token_id)


def _eq(a, b, what):
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert torch.equal(a, b) if a.dtype == torch.int64 else same_bits(a.contiguous(), b.contiguous()), what


@pytest.mark.parametrize("partial", [False, True])
def test_caption_stream_equals_greedy_decode(native, partial):
    m, cfg, cams, free, pcases = native
    F = cfg.mem_tokens
    pr = _rows(pcases["ragged"])
    st = m.caption_stream(batch=B, hop=1, max_len=L, stop="never", logprobs=True, partial=partial, prompt=pr)
    assert st.prompt_lengths.tolist() == [1, 3, 6]
    captions = 0
    for j in range(F + 2):
        if j == F + 1:
            pr = _rows(pcases["shared4"])
            st.prompt = pr                                          # replaced for the captions that follow
        out = st.push(cams[:, j])
        n = min(j + 1, F)
        if n < F and not partial:
            assert out is None
            continue
        win = cams[:, j + 1 - n:j + 1]
        src = win if n == F else [win[b] for b in range(B)]
        ref, ref_lp = m.greedy_decode(src, max_len=L, stop="never", return_logprobs=True, prompt=pr)
        _eq(out, ref, f"push {j + 1}")
        _eq(st.last_logprobs, ref_lp, f"logprobs of push {j + 1}")
        assert not torch.equal(ref, m.greedy_decode(src, max_len=L, stop="never"))
        captions += 1
    assert captions == (F + 2 if partial else 3)
    st.prompt = None
    assert st.prompt is None and st.prompt_lengths is None
    with pytest.raises(ValueError, match="carry=True is not combined"):
        m.caption_stream(batch=1, carry=True, max_len=L, prompt=[torch.tensor([5])])


def test_stream_pool_with_one_prompted_camera_equals_greedy_decode(native):
    m, cfg, cams, free, pcases = native
    F, sep = cfg.mem_tokens, cfg.sep_token_id
    pool = m.stream_pool(B, hop=1, max_len=L, logprobs=True)        # the model's stop rule: all_sep, cut per row
    prompt = torch.tensor(pcases["ragged"][2][1:])                  # without CLS: the pool prepends it
    pool.set_prompt(2, prompt)
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
            kw = dict(prompt=[prompt]) if c == 2 else {}
            pl = 6 if c == 2 else 1
            ref, ref_lp = m.greedy_decode(clip, max_len=L, stop="never", return_logprobs=True, **kw)
            hits = (ref[0, pl:] == sep).nonzero()
            k = pl - 1 + int(hits[0]) + 1 if hits.numel() else L
            _eq(ids, ref[0, :1 + k], f"camera {c} after {at[c]} frames")
            _eq(pool.last_logprobs[c], ref_lp[0, :k], f"logprobs of camera {c} after {at[c]} frames")
            assert pool.last_prompt_lengths[c] == pl
            if c == 2:
                differs |= not torch.equal(ref, m.greedy_decode(clip, max_len=L, stop="never"))
    assert differs and max(at) > F
    pool.set_prompt(2, None)
    out = pool.caption([2])
    ref = m.greedy_decode([cams[2, at[2] - F:at[2]]], max_len=L, stop="never")
    assert torch.equal(out[2].cpu(), ref[0, :out[2].shape[0]].cpu()) and pool.last_prompt_lengths[2] == 1


# ---- beam search ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["shared4", "ragged"])
def test_beam_search_equals_the_host_search(model, cases, name):
    m, cfg, mem, free = model
    prompts, _ = cases[name]
    base = m.beam_search(mem, max_len=L, k=K)
    dev = m.beam_search(mem, max_len=L, k=K, prompt=_rows(prompts))
    assert not torch.equal(dev, base)
    for b in range(B):                                              # clip by clip
        host = m.beam_search_host(mem[b:b + 1], max_len=L, k=K, prompt=_rows(prompts[b:b + 1]))
        assert torch.equal(dev[b:b + 1], host), (b, dev[b], host)
        assert dev[b, :len(prompts[b])].tolist() == prompts[b]
        assert torch.equal(m.beam_search(mem[b:b + 1], max_len=L, k=K, prompt=_rows(prompts[b:b + 1])), dev[b:b + 1])
    assert torch.equal(dev, m.beam_search_host(mem, max_len=L, k=K, prompt=_rows(prompts)))
    want = P.beam_yardstick(lambda ids, me: m.forward_decoder(ids.cuda(), me), mem, L, K, prompts, cfg.cls_token_id)
    assert np.array_equal(dev.cpu().numpy(), want)
    clips = [mem[0, :2], mem[1], mem[2, :3]]                        # ragged memories: every clip is the clip alone
    rag = m.beam_search(clips, max_len=L, k=K, prompt=_rows(prompts))
    for b, c in enumerate(clips):
        assert torch.equal(m.beam_search([c], max_len=L, k=K, prompt=_rows(prompts[b:b + 1])), rag[b:b + 1]), b
    assert torch.equal(m.beam_search(mem, max_len=L, k=K), base)
    kw = dict(no_repeat_ngram_size=2)
    assert torch.equal(m.beam_search(mem, max_len=L, k=K, prompt=_rows(prompts), **kw),
                       m.beam_search_host(mem, max_len=L, k=K, prompt=_rows(prompts), **kw))


def test_caption_stream_beams_take_the_prompt(native):
    m, cfg, cams, free, pcases = native
    F = cfg.mem_tokens
    pr = _rows(pcases["ragged"])
    st = m.caption_stream(batch=B, hop=1, max_len=9, beams=K, prompt=pr)
    for j in range(F + 1):
        out = st.push(cams[:, j])
        assert (out is None) == (j + 1 < F)
        if out is not None:
            win = cams[:, j + 1 - F:j + 1]
            assert torch.equal(out, m.beam_search(win, max_len=9, k=K, prompt=pr)), j
            assert torch.equal(out, m.beam_search_host(win, max_len=9, k=K, prompt=pr)), j


# ---- refusals and the life cycle -------------------------------------------------------------------------------------------------------

def test_life_cycle_refusals_and_workspace(model, cases):
    m, cfg, mem, free = model
    lib, h, V = m._lib, m._handle, cfg.vocab_length
    prompts, (want, _, _) = cases["ragged"]
    want = torch.as_tensor(want).cuda()
    tab, lens = P.table(prompts, cfg.cls_token_id)
    pid, pln = torch.as_tensor(tab).cuda(), torch.as_tensor(lens).cuda()
    ld = pid.shape[1]
    ids = torch.zeros((B, L + 1), dtype=torch.int64, device="cuda")
    steps = torch.zeros((1,), dtype=torch.int32, device="cuda")
    acc = ctypes.c_int32(-1)
    logits = torch.empty((B, 1, V), device="cuda")

    def greedy(max_len=L):
        rc = lib.gitcap_student_greedy(h, ptr(mem), B, max_len, 0, ptr(ids), ptr(steps), stream())
        torch.cuda.synchronize()
        return rc

    def attach(p=pid, n=pln, lo=1, hi=6, ldp=None):
        return lib.gitcap_student_attach_prompt(h, ptr(p), ld if ldp is None else ldp, ptr(n), lo, hi)
    assert attach() == 0 and attach(None, None) == 0                # NULL / NULL detaches
    assert greedy() == 0 and torch.equal(ids, free)
    assert attach() == 0
    # set_memory, forward_decoder and score leave it pending
    assert lib.gitcap_student_set_memory(h, ptr(mem), B, stream()) == 0
    assert lib.gitcap_student_forward_decoder(h, ptr(free[:, :1].contiguous()), 1, B, 1, ptr(logits), stream()) == 0
    m.score(mem, free)
    assert greedy() == 0 and torch.equal(ids, want)
    assert greedy() == 0 and torch.equal(ids, free)                 # consumed: the next call has no prompt
    assert attach() == 0 and greedy(max_len=99) == ERR_ARG          # a refused call consumes it
    assert greedy() == 0 and torch.equal(ids, free)
    assert attach() == 0 and greedy(max_len=5) == ERR_ARG           # the prompt's max_len 6 > the call's max_len
    assert b"longer than max_len" in lib.gitcap_student_last_error(h)
    assert greedy() == 0 and torch.equal(ids, free)
    best = torch.zeros((B, 6), dtype=torch.int64, device="cuda")
    assert attach() == 0                                            # beam: at least one free position
    assert lib.gitcap_student_beam_search(h, ptr(mem), B, K, 6, ptr(best), stream()) == ERR_ARG
    assert b"longer than max_len - 1" in lib.gitcap_student_last_error(h)
    # a draft call consumes it and refuses
    assert attach() == 0
    rc = lib.gitcap_student_greedy_draft(h, ptr(mem), B, ptr(free), L + 1, L, L, 0, ptr(ids), ptr(steps), ctypes.byref(acc), stream())
    assert rc == ERR_ARG and b"prompt" in lib.gitcap_student_last_error(h)
    assert greedy() == 0 and torch.equal(ids, free)
    for bad in (dict(n=None), dict(p=None), dict(lo=0), dict(lo=4, hi=3), dict(hi=ld + 1), dict(hi=14, ldp=14)):
        assert attach(**bad) == ERR_ARG, bad
    off = torch.zeros(ld * B + 1, dtype=torch.int64, device="cuda")
    assert lib.gitcap_student_attach_prompt(h, ctypes.c_void_p(off.data_ptr() + 4), ld, ptr(pln), 1, 6) == ERR_ARG
    assert greedy() == 0 and torch.equal(ids, free)                 # nothing was left attached; the handle is usable
    # lengths outside [1, max_len] are clamped on the device: 0 is no prompt, 99 the whole of the call's max_len columns
    odd = torch.tensor([0, 3, 99], dtype=torch.int32, device="cuda")
    wide = torch.cat([pid, pid.new_full((B, L - ld), 5)], 1).contiguous()
    assert lib.gitcap_student_attach_prompt(h, ptr(wide), L, ptr(odd), 1, L) == 0 and greedy() == 0
    assert torch.equal(ids[0], free[0]) and torch.equal(ids[1], want[1]) and ids[2, 1:L].tolist() == wide[2, 1:L].tolist()
    with pytest.raises(ValueError, match="draft= is not combined"):
        m.greedy_decode(mem, max_len=L, draft=free, prompt=_rows(prompts))
    with pytest.raises(ValueError, match="exceeds max_len"):
        m.greedy_decode(mem, max_len=5, prompt=_rows(prompts))
    with pytest.raises(ValueError, match="exceeds max_len - 1"):
        m.beam_search(mem, max_len=6, k=K, prompt=_rows(prompts))
    with pytest.raises(ValueError):
        m.greedy_decode(mem, max_len=L, prompt=_rows(prompts[:2]))
    assert greedy() == 0 and torch.equal(ids, free)


def test_a_handle_that_never_attaches_keeps_its_workspace():
    cfg = student_tiny()
    m = StudentCaptioner(cfg=cfg, weights=student_synthetic_weights(cfg, 0), **KW)
    mem = make_memory(B, cfg.mem_tokens, cfg.d_model, P.MEM_SEED).cuda()

    def ws():
        n = ctypes.c_int64(-1)
        assert m._lib.gitcap_student_workspace_bytes(m._handle, ctypes.byref(n)) == 0
        return int(n.value)
    w0 = ws()
    free = m.greedy_decode(mem, max_len=L)
    assert ws() == w0 and w0 > 0
    m.greedy_decode(mem, max_len=L, prompt=[torch.tensor([5, 6])] * B)
    w1 = ws()
    R, Tmax = KW["max_batch"], KW["max_text_len"] + 1
    assert w1 - w0 == R * (Tmax + 1) * 8 + R * 4                    # the two tables, once
    m.greedy_decode(mem, max_len=L, prompt=[torch.tensor([7])] * B)
    assert ws() == w1 and torch.equal(m.greedy_decode(mem, max_len=L), free)
