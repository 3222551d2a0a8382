"""Prompted decoding through the public surface (greedy_decode / infer / infer_async with prompt=, gitcap_attach_prompt) on git_tiny
with the seeded weights of tests/golden/: exact equality everywhere the same kernels run (self-consistency, a host-driven loop over
gitcap_text_forward, batch invariance, the two greedy plans, the one-shot life cycle), and the device search against the host
operator started from each clip's prompt (predictions equal, scores within 1e-4, as tests/test_search_options_e2e_gpu.py)."""
import ctypes

import pytest
import torch

from gitcap.config import git_tiny
from gitcap.weights import synthetic_weights
from gpu_support import captioner_cls, ptr, stream  # noqa: F401
from oracle.git_oracle import make_frames

pytestmark = pytest.mark.gpu

ERR_ARG = -1
B, F, L, BEAMS, PNB, LS, LP = 4, 2, 10, 4, 2, 8, 0.6
SEED = 1247                         # the frames of tests/test_search_options_e2e_gpu.py (its first two clips)
PROMPT_SEED = 3
KW = dict(beam_size=BEAMS, max_steps=LS, length_penalty=LP, per_node_beam_size=PNB)


@pytest.fixture(scope="module")
def model(captioner_cls):
    cfg = git_tiny(2)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=B, max_frames=F, max_text_len=12, max_beams=BEAMS, stop="never")
    fr = make_frames(B, F, cfg.image_size, SEED).cuda()
    c, lp = m.greedy_decode(fr, max_len=L, return_logprobs=True)
    return m, cfg, fr, c.clone(), lp.clone()


def _random_prompts(cfg, lengths, seed):
    g = torch.Generator().manual_seed(seed)
    rows = []
    for n in lengths:
        r = torch.randint(0, cfg.vocab_size, (n,), generator=g)
        r[r == cfg.sep_token_id] = (cfg.sep_token_id + 1) % cfg.vocab_size
        r[0] = cfg.cls_token_id
        rows.append(r)
    return rows


def test_self_consistency(model):
    m, cfg, fr, c, lp0 = model
    assert tuple(c.shape) == (B, L + 1)
    for k in (1, 2, L):
        got, lp = m.greedy_decode(fr, max_len=L, prompt=c[:, :k], return_logprobs=True)
        assert torch.equal(got, c), k
        assert bool((lp[:, :k - 1] == 0).all()) and torch.equal(lp[:, k - 1:].view(torch.int32), lp0[:, k - 1:].view(torch.int32)), k
    ks = [1, 3, 2, 5]
    got, lp = m.greedy_decode(fr, max_len=L, prompt=[c[b, :k] for b, k in enumerate(ks)], return_logprobs=True)
    assert torch.equal(got, c)
    for b, k in enumerate(ks):
        assert bool((lp[b, :k - 1] == 0).all()) and torch.equal(lp[b, k - 1:].view(torch.int32), lp0[b, k - 1:].view(torch.int32))
    # prompt_lengths over a dense tensor; a prompt without its CLS gets one
    got = m.greedy_decode(fr, max_len=L, prompt=c[:, :5], prompt_lengths=torch.tensor(ks))
    assert torch.equal(got, c)
    assert torch.equal(m.greedy_decode(fr, max_len=L, prompt=c[:, 1:3]), c)
    assert torch.equal(m.greedy_decode_async(fr, max_len=L, prompt=c[:, :3]).result(), c)


def test_off_policy_prompts_vs_host_driven_loop(model):
    m, cfg, fr, c, _ = model
    lens = [4, 1, 6, 2]
    prompts = _random_prompts(cfg, lens, PROMPT_SEED)
    got = m.greedy_decode(fr, max_len=L, prompt=prompts)
    lib, h = m._lib, m._handle
    ids = torch.zeros((B, L + 1), dtype=torch.int64, device="cuda")
    ids[:, 0] = cfg.cls_token_id
    assert lib.gitcap_encode(h, ptr(fr), B, F, None, stream()) == 0
    for t in range(L):
        assert lib.gitcap_text_forward(h, ptr(ids[:, t:]), L + 1, B, 1, t, 1, None, 0, ptr(ids[:, t + 1:]), L + 1, stream()) == 0
        for b, n in enumerate(lens):
            if t + 1 < n:
                ids[b, t + 1] = int(prompts[b][t + 1])
    torch.cuda.synchronize()
    assert torch.equal(got, ids)
    for b, n in enumerate(lens):
        assert torch.equal(got[b, :n].cpu(), prompts[b])
    assert not torch.equal(got[0], c[0])                     # the prompt changes the caption


def test_batch_invariance(model):
    m, cfg, fr, _, _ = model
    lens = [4, 1, 6, 2]
    prompts = _random_prompts(cfg, lens, PROMPT_SEED)
    got = m.greedy_decode(fr, max_len=L, prompt=prompts)
    for b in range(B):
        solo = m.greedy_decode(fr[b:b + 1], max_len=L, prompt=[prompts[b]])
        assert torch.equal(solo, got[b:b + 1]), b


def test_prefill_pass_and_forced_steps_agree(model):
    m, cfg, fr, _, _ = model
    P = 5
    prompts = torch.stack(_random_prompts(cfg, [P] * B, PROMPT_SEED + 1))
    a, lpa = m.greedy_decode(fr, max_len=L, prompt=prompts, return_logprobs=True)             # one pass over positions 0 .. P-1
    old = m._lib.gitcap_dbg_config(20, 0)
    try:
        b, lpb = m.greedy_decode(fr, max_len=L, prompt=prompts, return_logprobs=True)         # P - 1 forced token steps
    finally:
        m._lib.gitcap_dbg_config(20, old)
    assert old == 1 and torch.equal(a, b) and torch.equal(lpa.view(torch.int32), lpb.view(torch.int32))
    assert torch.equal(a[:, :P].cpu(), prompts) and bool((lpa[:, :P - 1] == 0).all()) and bool((lpa[:, P - 1:] < 0).all())
    ragged = m.greedy_decode(fr, max_len=L, prompt=prompts, prompt_lengths=torch.tensor([P, P, P, 1]))   # min_len 1: forced steps
    assert torch.equal(ragged[:3], a[:3])
    assert torch.equal(m.greedy_decode(fr, max_len=L, prompt=prompts, stop="all_sep")[:, :P].cpu(), prompts)


def _same_search(dev, host, lens):
    assert torch.equal(dev["predictions"].cpu(), host["predictions"].cpu()), (dev["predictions"], host["predictions"])
    err = (dev["logprobs"].cpu() - host["logprobs"].cpu()).abs().max().item()
    print(f"max |device - host operator| {err:.3e}")
    assert err <= 1e-4
    assert dev["prompt_lengths"].cpu().tolist() == lens and host["prompt_lengths"].cpu().tolist() == lens


def test_beam_search_vs_host_operator(model):
    m, cfg, fr, _, _ = model
    fr2 = fr[:2].contiguous()
    lens = [3, 2]
    prompts = _random_prompts(cfg, lens, PROMPT_SEED)
    dev = m.infer(fr2, on_device=True, prompt=prompts, **KW)
    host = m.infer(fr2, on_device=False, prompt=prompts, **KW)
    assert tuple(dev["predictions"].shape) == (2, LS)
    _same_search(dev, host, lens)
    for b, n in enumerate(lens):
        assert torch.equal(dev["predictions"][b, :n].cpu(), prompts[b])
    assert not torch.equal(dev["predictions"], m.infer(fr2, on_device=True, **KW)["predictions"])
    opt = dict(num_keep_best=3, repetition_penalty=1.2)
    dev3 = m.infer(fr2, on_device=True, prompt=prompts, **KW, **opt)
    _same_search(dev3, m.infer(fr2, on_device=False, prompt=prompts, **KW, **opt), lens)
    assert tuple(dev3["predictions"].shape) == (2, 3, LS)
    sub = m.infer_async(fr2, prompt=prompts, **KW, **opt).result()
    assert torch.equal(sub["predictions"], dev3["predictions"]) and torch.equal(sub["logprobs"], dev3["logprobs"])
    assert sub["prompt_lengths"].tolist() == lens
    for b in range(2):                                        # a clip alone == the clip inside the ragged batch
        solo = m.infer(fr2[b:b + 1], on_device=True, prompt=[prompts[b]], **KW)
        assert torch.equal(solo["predictions"], dev["predictions"][b:b + 1]) and torch.equal(solo["logprobs"], dev["logprobs"][b:b + 1])


def test_entry_errors_and_one_shot(model):
    m, cfg, fr, c, _ = model
    lib, h = m._lib, m._handle
    pr = torch.stack(_random_prompts(cfg, [6] * B, 9)).cuda()
    lens = torch.full((B,), 6, dtype=torch.int32, device="cuda")

    def greedy(max_len=L, stop=0):
        ids = torch.full((B, max_len + 1), -7, dtype=torch.int64, device="cuda")
        rc = lib.gitcap_greedy(h, ptr(fr), B, F, max_len, stop, ptr(ids), None, stream())
        torch.cuda.synchronize()
        return rc, ids
    # a prompt longer than the call's max_len: refused, nothing written, and consumed
    assert lib.gitcap_attach_prompt(h, ptr(pr), 6, ptr(lens), 6, 6) == 0
    rc, ids = greedy(max_len=4)
    assert rc == ERR_ARG and b"prompt" in lib.gitcap_last_error(h) and bool((ids == -7).all())
    rc, ids = greedy()
    assert rc == 0 and torch.equal(ids, c)
    # an attachment followed by a call refused for another reason does not leak into the call after it
    assert lib.gitcap_attach_prompt(h, ptr(pr), 6, ptr(lens), 6, 6) == 0
    rc, _ = greedy(stop=7)
    assert rc == ERR_ARG
    rc, ids = greedy()
    assert rc == 0 and torch.equal(ids, c)
    # honoured by the C call, and once only
    assert lib.gitcap_attach_prompt(h, ptr(pr), 6, ptr(lens), 6, 6) == 0
    rc, ids = greedy()
    assert rc == 0 and torch.equal(ids[:, :6], pr) and torch.equal(ids, m.greedy_decode(fr, max_len=L, prompt=pr))
    rc, ids = greedy()
    assert rc == 0 and torch.equal(ids, c)
    # the beam family consumes it as well: longer than max_steps - 1 is refused
    dec = torch.full((B, 6), -7, dtype=torch.int64, device="cuda")
    lp = torch.zeros((B,), device="cuda")
    assert lib.gitcap_attach_prompt(h, ptr(pr), 6, ptr(lens), 6, 6) == 0
    assert lib.gitcap_beam_search(h, ptr(fr), B, F, BEAMS, 6, ctypes.c_float(LP), PNB, ptr(dec), ptr(lp), stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((dec == -7).all())
    rc, ids = greedy()
    assert rc == 0 and torch.equal(ids, c)
    # refused attachments leave nothing pending; NULL, NULL detaches
    for bad in ((None, 6, ptr(lens), 6, 6), (ptr(pr), 6, None, 6, 6), (ptr(pr), 6, ptr(lens), 0, 6), (ptr(pr), 6, ptr(lens), 4, 3),
                (ptr(pr), 5, ptr(lens), 6, 6)):
        assert lib.gitcap_attach_prompt(h, *bad) == ERR_ARG, bad
    assert lib.gitcap_attach_prompt(h, ptr(pr), 6, ptr(lens), 6, 6) == 0 and lib.gitcap_attach_prompt(h, None, 0, None, 0, 0) == 0
    rc, ids = greedy()
    assert rc == 0 and torch.equal(ids, c)
    with pytest.raises(ValueError):
        m.greedy_decode(fr, max_len=4, prompt=pr)
    with pytest.raises(ValueError):
        m.infer(fr, prompt=pr, **dict(KW, max_steps=6))
