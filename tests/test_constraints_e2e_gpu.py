"""Constrained decoding end to end on the tiny model: the device loops under no_repeat_ngram_size / min_length / suppress_tokens
against a host loop over forward_decoder + the restatement (greedy: exact ids, a cached step being bit for bit the teacher-forced
position) and against the host search operator with the same options (beam family)."""
import ctypes
import dataclasses

import numpy as np
import pytest
import torch

import constraints_reference as C
import logprob_reference as LPR
from gitcap import _lib
from gitcap.config import git_tiny
from gitcap.weights import synthetic_weights
from gpu_support import captioner_cls, ptr, stream  # noqa: F401
from oracle.git_oracle import make_frames

pytestmark = pytest.mark.gpu

ERR_ARG = -1
B, F, L, BEAMS, PNB, LS, LP = 3, 2, 10, 4, 2, 8, 0.6
SEED = 1247
TOL = 2e-5                          # tests/test_logprob_gpu.py derives it
KW = dict(beam_size=BEAMS, max_steps=LS, length_penalty=LP, per_node_beam_size=PNB)


@pytest.fixture(scope="module")
def model(captioner_cls):
    cfg = git_tiny(2)
    w = synthetic_weights(cfg, 0)
    kw = dict(max_batch=4, max_frames=F, max_text_len=12, max_beams=BEAMS, stop="never")
    fr = make_frames(B, F, cfg.image_size, SEED).cuda()
    free = captioner_cls(cfg, w, **kw).greedy_decode(fr, max_len=L)
    # SEP = a token the unconstrained caption emits early, so that min_length changes the caption
    cfg = dataclasses.replace(cfg, sep_token_id=int(free[0, 2]))
    m = captioner_cls(cfg, w, **kw)
    free = m.greedy_decode(fr, max_len=L).clone()
    return m, cfg, fr, free


def _host_loop(m, cfg, fr, n, mlen, sup, prompts=None):
    """forward_decoder on the growing prefix -> mask_logits -> first arg-max; -> (ids, the log-probability restatement per step)"""
    Bn, V = fr.shape[0], cfg.vocab_size
    _, vis = m.forward_image_enc(fr)
    ids = np.full((Bn, L + 1), cfg.cls_token_id, dtype=np.int64)
    lps = np.zeros((Bn, L))
    for t in range(L):
        lg = m.forward_decoder(torch.as_tensor(ids[:, :t + 1]).cuda(), vis)[:, -1].float().cpu().numpy()
        masked = C.mask_logits(lg, C.ban_mask(ids, t + 1, n, mlen, cfg.sep_token_id, sup, V))
        tok, lp = LPR.token_logprobs(masked)
        for b in range(Bn):
            forced = prompts is not None and t + 1 < len(prompts[b])
            ids[b, t + 1] = int(prompts[b][t + 1]) if forced else int(np.argmax(masked[b]))
            assert forced or ids[b, t + 1] == tok[b]
            lps[b, t] = 0.0 if forced else lp[b]
    return torch.as_tensor(ids), lps


CASES = [dict(no_repeat_ngram_size=1), dict(no_repeat_ngram_size=2, min_length=6), dict(min_length=L + 1),
         dict(no_repeat_ngram_size=3, min_length=4, suppress_tokens="own")]


def _kw(case, free):
    kw = dict(case)
    if kw.get("suppress_tokens") == "own":                  # from the unconstrained caption's own tokens
        kw["suppress_tokens"] = sorted({int(free[0, 1]), int(free[1, 3]), int(free[2, 2])})
    return kw


@pytest.mark.parametrize("case", CASES)
def test_greedy_equals_the_host_loop_from_every_entry_point(model, case):
    m, cfg, fr, free = model
    kw = _kw(case, free)
    want, want_lp = _host_loop(m, cfg, fr, kw.get("no_repeat_ngram_size", 0), kw.get("min_length", 0), kw.get("suppress_tokens", []))
    got = m.greedy_decode(fr, max_len=L, **kw)
    assert torch.equal(got.cpu(), want), (got, want)
    assert not torch.equal(got, free)                       # the case bites
    for b in range(B):                                      # rows alone
        assert torch.equal(m.greedy_decode(fr[b:b + 1], max_len=L, **kw), got[b:b + 1]), b
    ids2, lp = m.greedy_decode(fr, max_len=L, return_logprobs=True, **kw)
    assert torch.equal(ids2, got)
    err = np.abs(lp.cpu().numpy().astype(np.float64) - want_lp).max()
    print(f"{kw}: max |log-probability - restatement over the masked row| {err:.3e}")
    assert err <= TOL
    # two submissions in flight with different constraints
    other = dict(no_repeat_ngram_size=1)
    f1 = m.greedy_decode_async(fr, max_len=L, **kw)
    f2 = m.greedy_decode_async(fr, max_len=L, **other)
    f3 = m.greedy_decode_async(fr, max_len=L)
    assert torch.equal(f1.result(), got) and torch.equal(f2.result(), m.greedy_decode(fr, max_len=L, **other)) and torch.equal(f3.result(), free)
    st = m.caption_stream(batch=B, window=F, max_len=L, stop="never", **kw)
    assert torch.equal(st.push(fr), got)
    assert torch.equal(m.greedy_decode(fr, max_len=L), free)          # the call after the consuming one is unconstrained
    seq = got.cpu().tolist()
    n = kw.get("no_repeat_ngram_size", 0)
    for b in range(B):
        assert not (n and C.repeats_ngram(seq[b], n))
        assert not set(seq[b]) & set(kw.get("suppress_tokens", []))
        assert cfg.sep_token_id not in seq[b][:kw.get("min_length", 0)]


def test_greedy_ragged_prompts_are_forced_even_when_banned(model):
    m, cfg, fr, free = model
    tok = int(free[0, 1])
    prompts = [torch.tensor([cfg.cls_token_id, tok, tok, 5, tok]), torch.tensor([cfg.cls_token_id]),
               torch.tensor([cfg.cls_token_id, cfg.sep_token_id, 7])]
    kw = dict(no_repeat_ngram_size=1, min_length=6, suppress_tokens=[5, 7])
    want, _ = _host_loop(m, cfg, fr, 1, 6, [5, 7], prompts)
    got = m.greedy_decode(fr, max_len=L, prompt=prompts, **kw)
    assert torch.equal(got.cpu(), want), (got, want)
    for b, p in enumerate(prompts):
        assert torch.equal(got[b, :len(p)].cpu(), p)
        tail = got[b, len(p):].cpu().tolist()
        assert not set(tail) & (set(p.tolist()) | {5, 7}) and len(set(tail)) == len(tail)     # the bans count the prompt's tokens
    assert torch.equal(m.greedy_decode_async(fr, max_len=L, prompt=prompts, **kw).result(), got)


def _same_search(dev, host):
    assert torch.equal(dev["predictions"].cpu(), host["predictions"].cpu()), (dev["predictions"], host["predictions"])
    err = (dev["logprobs"].cpu() - host["logprobs"].cpu()).abs().max().item()
    print(f"max |device - host operator| {err:.3e}")
    assert err <= 1e-4                                      # the bound tests/test_prompt_e2e_gpu.py holds the two searches to


@pytest.mark.parametrize("opt", [dict(), dict(num_keep_best=2, repetition_penalty=1.3)])
def test_beam_family_equals_the_host_operator(model, opt):
    m, cfg, fr, free = model
    fr2 = fr[:2].contiguous()
    base = m.infer(fr2, on_device=True, **KW, **opt)
    sup = sorted({int(v) for v in base["predictions"].reshape(-1, LS)[:, 1:3].reshape(-1).tolist()} - {cfg.sep_token_id})
    # (clip 0's unconstrained search ends at once: SEP is its second token, so a min_length bites; so do the clips' own tokens)
    for kw in (dict(no_repeat_ngram_size=1, min_length=5), dict(no_repeat_ngram_size=2, min_length=LS - 1, suppress_tokens=sup)):
        dev = m.infer(fr2, on_device=True, **KW, **opt, **kw)
        host = m.infer(fr2, on_device=False, **KW, **opt, **kw)
        _same_search(dev, host)
        assert not torch.equal(dev["predictions"], base["predictions"])
        sub = m.infer_async(fr2, **KW, **opt, **kw).result()
        assert torch.equal(sub["predictions"], dev["predictions"]) and torch.equal(sub["logprobs"], dev["logprobs"])
        st = m.caption_stream(batch=2, window=F, max_len=LS, beam_size=BEAMS, length_penalty=LP, per_node_beam_size=PNB, **opt, **kw)
        out = st.push(fr2)
        assert torch.equal(out["predictions"], dev["predictions"]) and torch.equal(out["logprobs"], dev["logprobs"])
    assert torch.equal(m.infer(fr2, on_device=True, **KW, **opt)["predictions"], base["predictions"])


def test_sampled_search_respects_the_constraints(model):
    m, cfg, fr, free = model
    fr2 = fr[:2].contiguous()
    sup = [int(free[0, 1]), int(free[1, 1])]
    kw = dict(no_repeat_ngram_size=2, min_length=5, suppress_tokens=sup, do_sample=True, top_k=20, temperature=1.2, seed=77)
    a = m.infer(fr2, on_device=True, **KW, **kw)
    b = m.infer(fr2, on_device=True, **KW, **kw)
    assert torch.equal(a["predictions"], b["predictions"]) and torch.equal(a["logprobs"], b["logprobs"])
    for seq in a["predictions"].cpu().tolist():
        end = seq.index(cfg.sep_token_id, 1) + 1 if cfg.sep_token_id in seq[1:] else len(seq)
        body = seq[:end]
        assert not C.repeats_ngram(body, 2) and not set(body) & set(sup), seq
        assert cfg.sep_token_id not in seq[1:5], seq


def test_life_cycle_and_errors(model):
    m, cfg, fr, free = model
    lib, h, V = m._lib, m._handle, cfg.vocab_size
    ids = torch.zeros((B, L + 1), dtype=torch.int64, device="cuda")
    steps = torch.zeros((1,), dtype=torch.int32, device="cuda")
    sup = torch.tensor([int(free[0, 1]), int(free[1, 1]), int(free[2, 1])], dtype=torch.int32, device="cuda")
    c = _lib.CConstraints(1, 0, sup.data_ptr(), 3)

    def greedy(max_len=L):
        rc = lib.gitcap_greedy(h, ptr(fr), B, F, max_len, 0, ptr(ids), ptr(steps), stream())
        torch.cuda.synchronize()
        return rc
    assert lib.gitcap_attach_constraints(h, ctypes.byref(c)) == 0 and lib.gitcap_attach_constraints(h, None) == 0
    ws0 = m.workspace_bytes()                               # the masks exist from the first attach on, and are counted once
    assert lib.gitcap_attach_constraints(h, ctypes.byref(c)) == 0
    assert m.workspace_bytes() == ws0
    assert lib.gitcap_encode(h, ptr(fr), B, F, None, stream()) == 0          # a non-family call leaves it pending
    assert greedy() == 0 and not torch.equal(ids, free)
    constrained = ids.clone()
    assert greedy() == 0 and torch.equal(ids, free)         # consumed: the next call is unconstrained
    assert lib.gitcap_attach_constraints(h, ctypes.byref(c)) == 0
    assert greedy(max_len=99) == ERR_ARG                    # a refused call consumes it
    assert greedy() == 0 and torch.equal(ids, free)
    assert lib.gitcap_attach_constraints(h, ctypes.byref(c)) == 0
    assert lib.gitcap_attach_constraints(h, None) == 0      # NULL detaches
    assert greedy() == 0 and torch.equal(ids, free)
    for bad in (_lib.CConstraints(-1, 0, None, 0), _lib.CConstraints(0, -1, None, 0), _lib.CConstraints(0, 0, None, -1),
                _lib.CConstraints(0, 0, sup.data_ptr(), 257), _lib.CConstraints(0, 0, None, 2), _lib.CConstraints(0, 0, sup.data_ptr() + 2, 2)):
        assert lib.gitcap_attach_constraints(h, ctypes.byref(bad)) == ERR_ARG
    assert greedy() == 0 and torch.equal(ids, free)         # nothing was left attached; the handle is usable
    many = torch.arange(V - L, dtype=torch.int32, device="cuda")[:256]
    if many.numel() + L >= V:                               # n_suppress + max_len >= vocab_size: refused at the consuming call
        big = _lib.CConstraints(0, 0, many.data_ptr(), many.numel())
        assert lib.gitcap_attach_constraints(h, ctypes.byref(big)) == 0
        assert greedy() == ERR_ARG
        assert greedy() == 0 and torch.equal(ids, free)
    with pytest.raises(ValueError):
        m.greedy_decode(fr, max_len=L, no_repeat_ngram_size=-1)
    with pytest.raises(ValueError):
        m.greedy_decode(fr, max_len=L, min_length=-1)
    with pytest.raises(ValueError):
        m.greedy_decode(fr, max_len=L, suppress_tokens=list(range(257)))
    with pytest.raises(ValueError):
        m.infer(fr[:2], suppress_tokens=list(range(V - LS)), **KW)
    with pytest.raises(ValueError):
        m.greedy_decode_async(fr, max_len=L, suppress_tokens=list(range(V - L)))
    assert lib.gitcap_attach_constraints(h, ctypes.byref(c)) == 0
    assert greedy() == 0 and torch.equal(ids, constrained)
    assert torch.equal(m.greedy_decode(fr, max_len=L), free)
