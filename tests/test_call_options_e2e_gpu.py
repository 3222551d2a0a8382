"""The life cycle of the one-shot attachments across call families (include/gitcap.h: gitcap_attach_*): an attachment waits
through the calls that do not take it and is consumed by the first call that does.  The per-feature suites pin each attachment
with its own family; this file pins the cross-family rows: log-probabilities wait through a beam search, search options through a
greedy call, prompt and constraints through gitcap_encode -- and a ragged batch that carries every option at once gives the
same results submitted as synchronously, from device clips and from host clips.

git_tiny(num_frames=3): up to 3 clips of up to 3 frames, max_len 6, 2 beams x 2 candidates."""
import ctypes

import pytest
import torch

from gpu_support import NAN, captioner_cls, poisoned, ptr, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu

COUNTS = [2, 3, 1]
MAX_LEN = 6
IDS_FILL = -777
PROMPT = [[5, 9], [], [7]]
CONS = dict(no_repeat_ngram_size=2, min_length=4, suppress_tokens=[11, 12])


@pytest.fixture(scope="module")
def tiny(captioner_cls):
    from gitcap.config import git_tiny
    from gitcap.weights import synthetic_weights
    cfg = git_tiny(num_frames=3)
    m = captioner_cls(cfg, synthetic_weights(cfg, seed=0), device="cuda:0", max_batch=3, max_frames=3, max_text_len=8, max_beams=2)
    g = torch.Generator().manual_seed(21)
    clips = [torch.randn(n, 3, cfg.image_size, cfg.image_size, generator=g) for n in COUNTS]
    x = torch.randn(3, 3, 3, cfg.image_size, cfg.image_size, generator=g).cuda()
    return m, clips, x


def _greedy(m, x, ids):
    m._call("gitcap_greedy", ptr(x), x.shape[0], x.shape[1], MAX_LEN, 0, ptr(ids), None, m._stream())
    torch.cuda.synchronize()


def _beam(m, x, decoded, logprobs):
    m._call("gitcap_beam_search", ptr(x), x.shape[0], x.shape[1], 2, MAX_LEN, ctypes.c_float(0.6), 2, ptr(decoded), ptr(logprobs), m._stream())
    torch.cuda.synchronize()


def _beam_buffers(B):
    return torch.empty((B, MAX_LEN), dtype=torch.int64, device="cuda"), torch.empty((B,), dtype=torch.float32, device="cuda")


def test_token_logprobs_wait_through_a_beam_search(tiny):
    m, _, x = tiny
    B = x.shape[0]
    ref_ids, ref_lp = m.greedy_decode(x, max_len=MAX_LEN, stop="never", return_logprobs=True)
    ref_beam = m.infer(x, beam_size=2, max_steps=MAX_LEN)
    lp = poisoned((B, MAX_LEN), NAN)
    m._call("gitcap_attach_token_logprobs", ptr(lp), MAX_LEN)
    decoded, logprobs = _beam_buffers(B)
    _beam(m, x, decoded, logprobs)
    assert bool(torch.isnan(lp).all())                       # the beam call left the buffer alone ...
    assert torch.equal(decoded, ref_beam["predictions"]) and same_bits(logprobs, ref_beam["logprobs"][:, 0].contiguous())
    ids = torch.empty((B, MAX_LEN + 1), dtype=torch.int64, device="cuda")
    _greedy(m, x, ids)
    assert torch.equal(ids, ref_ids) and same_bits(lp, ref_lp.contiguous())      # ... and the greedy call behind it fills it
    lp2 = poisoned((B, MAX_LEN), NAN)                        # consumed: a second greedy call writes nothing more
    lp.copy_(lp2)
    _greedy(m, x, ids)
    assert bool(torch.isnan(lp).all())


def test_search_options_wait_through_a_greedy_call(tiny):
    from gitcap._lib import CSearchOptions
    m, _, x = tiny
    B = x.shape[0]
    ref_ids = m.greedy_decode(x, max_len=MAX_LEN, stop="never")
    ref = m.infer(x, beam_size=2, max_steps=MAX_LEN, num_keep_best=2)
    nbest = poisoned((B, 2, MAX_LEN), IDS_FILL, torch.int64)
    nbest_lp = poisoned((B, 2), NAN)
    opt = CSearchOptions(2, 1.0, nbest.data_ptr(), nbest_lp.data_ptr())
    m._call("gitcap_attach_search_options", ctypes.byref(opt))
    ids = torch.empty((B, MAX_LEN + 1), dtype=torch.int64, device="cuda")
    _greedy(m, x, ids)
    assert torch.equal(ids, ref_ids)
    assert bool((nbest == IDS_FILL).all()) and bool(torch.isnan(nbest_lp).all())     # the greedy call left the options pending
    decoded, logprobs = _beam_buffers(B)
    _beam(m, x, decoded, logprobs)
    assert torch.equal(nbest, ref["predictions"]) and same_bits(nbest_lp, ref["logprobs"].contiguous())
    assert torch.equal(decoded, nbest[:, 0]) and same_bits(logprobs, nbest_lp[:, 0].contiguous())
    nbest.fill_(IDS_FILL)                                    # consumed: the next search keeps one hypothesis
    _beam(m, x, decoded, logprobs)
    assert bool((nbest == IDS_FILL).all())


def test_prompt_and_constraints_wait_through_an_encode(tiny):
    from gitcap._lib import CConstraints
    m, _, x = tiny
    B, F = x.shape[:2]
    pids = torch.tensor([[101, 5, 9], [101, 101, 101], [101, 7, 101]], dtype=torch.int64, device="cuda")
    plen = torch.tensor([3, 1, 2], dtype=torch.int32, device="cuda")
    sup = torch.tensor(CONS["suppress_tokens"], dtype=torch.int32, device="cuda")
    cons = CConstraints(CONS["no_repeat_ngram_size"], CONS["min_length"], sup.data_ptr(), sup.numel())
    pids[:, 0] = m.cls_token_id

    def attach():
        m._call("gitcap_attach_prompt", ptr(pids), pids.shape[1], ptr(plen), 1, 3)
        m._call("gitcap_attach_constraints", ctypes.byref(cons))

    plain = torch.empty((B, MAX_LEN + 1), dtype=torch.int64, device="cuda")
    _greedy(m, x, plain)
    direct = torch.empty_like(plain)
    attach()
    _greedy(m, x, direct)
    assert torch.equal(direct[0, :3], pids[0]) and torch.equal(direct[2, :2], pids[2, :2]) and not torch.equal(direct, plain)
    ref = m.greedy_decode(x, max_len=MAX_LEN, stop="never", prompt=[[5, 9], [], [7]], **CONS)
    assert torch.equal(direct, ref)
    vis = torch.empty((B, F * m.cfg.tokens_per_frame, m.cfg.enc_width), dtype=torch.float32, device="cuda")
    behind = torch.empty_like(plain)
    attach()
    m._call("gitcap_encode", ptr(x), B, F, ptr(vis), m._stream())
    _greedy(m, x, behind)
    assert torch.equal(behind, direct)
    again = torch.empty_like(plain)                          # consumed: the next call is the plain one
    _greedy(m, x, again)
    assert torch.equal(again, plain)


@pytest.mark.parametrize("host", [False, True], ids=["device", "host"])
def test_ragged_async_with_every_option_equals_the_synchronous_call(tiny, host):
    m, clips, _ = tiny
    src = clips if host else [c.cuda() for c in clips]
    prompt = [torch.tensor(p, dtype=torch.int64) for p in PROMPT]
    gkw = dict(max_len=MAX_LEN, stop="never", prompt=prompt, **CONS)
    ref = m.greedy_decode(src, **gkw)
    futs = [m.greedy_decode_async(src, **gkw) for _ in range(2)]
    ikw = dict(beam_size=2, max_steps=MAX_LEN, per_node_beam_size=2, num_keep_best=2, do_sample=True, top_k=5, temperature=0.9, seed=1234,
               prompt=prompt, **CONS)
    iref = m.infer(src, **ikw)
    ifuts = [m.infer_async(src, **ikw) for _ in range(2)]
    for f in futs:
        ids = f.result()
        assert ids.device == ref.device and torch.equal(ids, ref)
    assert not torch.equal(ref, m.greedy_decode(src, max_len=MAX_LEN, stop="never"))      # (the options did bear on the result)
    for f in ifuts:
        r = f.result()
        assert r["predictions"].shape == (3, 2, MAX_LEN) and torch.equal(r["predictions"].cpu(), iref["predictions"].cpu())
        assert same_bits(r["logprobs"].cpu().contiguous(), iref["logprobs"].cpu().contiguous())
        assert r["seed"] == iref["seed"] == 1234
        assert r["prompt_lengths"].tolist() == iref["prompt_lengths"].tolist() == [3, 1, 2]
