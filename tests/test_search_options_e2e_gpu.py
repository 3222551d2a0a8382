"""num_keep_best and repetition_penalty of the device-resident search through the public surface (gitcap_attach_search_options,
infer / infer_async / caption_stream) on git_tiny with the seeded weights the fixtures of tests/golden/ were made with.

Reference: the host-side operator (infer(on_device=False), gitcap/search.py) on the same handle -- predictions equal, scores within
1e-4.  The frames' seed was chosen on the CPU (oracle.git_oracle.GitOracle under oracle.search_oracle.beam_search) so that the
candidates of every step are more than 5e-3 apart; the test recomputes that gap from the logits the device search saved and fails if
it is below 1e-3.  Everything else is torch.equal: the result does not depend on the entry point or on the batch beside a clip."""
import ctypes

import numpy as np
import pytest
import torch

import search_options_reference as S
from gitcap.config import git_tiny
from gitcap.weights import synthetic_weights
from gpu_support import camera, captioner_cls, ptr, stream  # noqa: F401
from oracle.git_oracle import make_frames

pytestmark = pytest.mark.gpu

ERR_ARG = -1
B, F, BEAMS, PNB, L, N, RP, LP = 2, 2, 4, 2, 8, 3, 1.3, 0.6
SEED = 1247
KW = dict(beam_size=BEAMS, max_steps=L, length_penalty=LP, per_node_beam_size=PNB)
OPT = dict(num_keep_best=N, repetition_penalty=RP)


@pytest.fixture(scope="module")
def model(captioner_cls):
    cfg = git_tiny(2)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=B, max_frames=F, max_text_len=L, max_beams=BEAMS, stop="never")
    fr = make_frames(B, F, cfg.image_size, SEED).cuda()
    ws0 = m.workspace_bytes()
    r = m.infer(fr, on_device=True, **KW)                  # before any attachment
    before = (r["predictions"].clone(), r["logprobs"].clone())
    r = m.infer(fr, on_device=True, **KW, **OPT)
    dev = (r["predictions"].clone(), r["logprobs"].clone())
    return m, cfg, fr, before, dev, ws0


def _c_search(m, fr, opt=None, beams=BEAMS, nb=B, fill=-777):
    """One synchronous gitcap_beam_search, optionally behind an attachment with poisoned n-best buffers."""
    from gitcap._lib import CSearchOptions
    dec = torch.full((nb, L), fill, dtype=torch.int64, device="cuda")
    lp = torch.full((nb,), float("nan"), device="cuda")
    nbest = torch.full((nb, 16, L), fill, dtype=torch.int64, device="cuda")
    nlp = torch.full((nb, 16), float("nan"), device="cuda")
    rc_attach = None
    if opt is not None:
        n, rp = opt
        o = CSearchOptions(n, rp, nbest.data_ptr(), nlp.data_ptr())
        rc_attach = m._lib.gitcap_attach_search_options(m._handle, ctypes.byref(o))
    rc = m._lib.gitcap_beam_search(m._handle, ptr(fr), nb, F, beams, L, ctypes.c_float(LP), PNB, ptr(dec), ptr(lp), stream())
    torch.cuda.synchronize()
    return rc_attach, rc, dec, lp, nbest, nlp


def test_device_search_with_options_vs_host_operator(model):
    m, cfg, fr, before, dev, _ = model
    pred, lps = dev
    assert tuple(pred.shape) == (B, N, L) and pred.dtype == torch.int64 and tuple(lps.shape) == (B, N) and lps.dtype == torch.float32
    host = m.infer(fr, on_device=False, **KW, **OPT)
    # the input condition, from the device's own logits: every step's candidates are apart
    saved = m.infer(fr, on_device=True, save_logits=True, **KW, **OPT)
    assert torch.equal(saved["predictions"], pred) and torch.equal(saved["logprobs"], lps)
    steps = saved["logits_dict"]
    assert tuple(steps.shape) == (L - 1, B * BEAMS, cfg.vocab_size)
    r_dec, r_lp, gap = S.replay_search(steps.cpu().numpy(), B, BEAMS, BEAMS * PNB, L, cfg.sep_token_id, cfg.cls_token_id, LP, N, RP)
    err_host = (lps - host["logprobs"].to(lps.device)).abs().max().item()
    err_replay = np.abs(lps.cpu().numpy() - r_lp).max()
    print(f"candidate gap {gap:.3e}; max |device - host operator| {err_host:.3e}; max |device - replay of its logits| {err_replay:.3e}")
    assert gap > 1e-3, gap
    assert torch.equal(pred.cpu(), host["predictions"].cpu())
    assert err_host <= 1e-4
    assert np.array_equal(pred.cpu().numpy(), r_dec) and err_replay <= 1e-4
    # ranked, CLS first, and the options do something on these frames
    assert bool((pred[:, :, 0] == cfg.cls_token_id).all()) and bool((lps[:, :-1] >= lps[:, 1:]).all())
    plain3 = m.infer(fr, on_device=True, **KW, num_keep_best=N)
    assert not torch.equal(plain3["predictions"], pred)                       # the penalty changes a caption
    assert tuple(m.infer(fr, on_device=True, **KW, repetition_penalty=RP)["predictions"].shape) == (B, L)


def test_every_entry_point_gives_the_same_bits(model):
    m, cfg, fr, before, dev, _ = model
    from gitcap.preprocess import preprocess_frames
    r = m.infer(fr, **KW, **OPT)                                               # the default is the device search now
    assert torch.equal(r["predictions"], dev[0]) and torch.equal(r["logprobs"], dev[1])
    futs = [m.infer_async(fr, **KW, **OPT), m.infer_async(fr, **KW), m.infer_async(fr, **KW, **OPT)]     # in flight together
    got = [f.result() for f in futs]
    for g in (got[0], got[2]):
        assert torch.equal(g["predictions"], dev[0]) and torch.equal(g["logprobs"], dev[1])
    assert torch.equal(got[1]["predictions"], before[0]) and torch.equal(got[1]["logprobs"], before[1])
    s = m.caption_stream(batch=B, window=F, max_len=L, **{k: v for k, v in KW.items() if k != "max_steps"}, **OPT)
    w = s.push(fr)
    assert torch.equal(w["predictions"], dev[0]) and torch.equal(w["logprobs"], dev[1])
    # raw camera frames: the raw submission == the transform followed by the plain call
    cam = camera((B, F, 80, 96, 3), 5).cuda()
    pre = preprocess_frames(cam, cfg.image_size).contiguous()
    a, b = m.infer(cam, on_device=True, **KW, **OPT), m.infer(pre, on_device=True, **KW, **OPT)
    c = m.infer_async(cam, **KW, **OPT).result()
    assert tuple(a["predictions"].shape) == (B, N, L)
    for x in (b, c):
        assert torch.equal(a["predictions"], x["predictions"]) and torch.equal(a["logprobs"], x["logprobs"])
    # CPU frames in -> CPU results out
    h = m.infer_async(fr.cpu(), **KW, **OPT).result()
    assert h["predictions"].device.type == "cpu" and torch.equal(h["predictions"], dev[0].cpu()) and torch.equal(h["logprobs"], dev[1].cpu())


def test_c_outputs_rank0_and_one_slot(model):
    m, cfg, fr, before, dev, _ = model
    ra, rc, dec, lp, nbest, nlp = _c_search(m, fr, (N, RP))
    assert ra == 0 and rc == 0
    assert torch.equal(nbest.view(-1)[:B * N * L].view(B, N, L), dev[0]) and torch.equal(nlp.view(-1)[:B * N].view(B, N), dev[1])
    assert bool((nbest.view(-1)[B * N * L:] == -777).all()) and bool(torch.isnan(nlp.view(-1)[B * N:]).all())    # nothing behind [B][n]
    assert torch.equal(dec, dev[0][:, 0]) and torch.equal(lp, dev[1][:, 0])                                     # the call's own outputs: rank 0
    # n = 1 with a penalty: the pointers may be NULL; given, they receive a copy
    from gitcap._lib import CSearchOptions
    o = CSearchOptions(1, RP, None, None)
    assert m._lib.gitcap_attach_search_options(m._handle, ctypes.byref(o)) == 0
    _, rc, dec1, lp1, _, _ = _c_search(m, fr)
    assert rc == 0
    ra, rc, dec2, lp2, nbest, nlp = _c_search(m, fr, (1, RP))
    assert ra == 0 and rc == 0 and torch.equal(dec1, dec2) and torch.equal(lp1, lp2)
    assert torch.equal(nbest.view(-1)[:B * L].view(B, L), dec1) and torch.equal(nlp.view(-1)[:B], lp1)
    r = m.infer(fr, on_device=True, **KW, repetition_penalty=RP)
    assert torch.equal(r["predictions"], dec1) and torch.equal(r["logprobs"][:, 0], lp1)


def test_attachment_is_one_shot_and_checked(model):
    m, cfg, fr, before, dev, _ = model
    lib, h = m._lib, m._handle
    from gitcap._lib import CSearchOptions
    # consumed by a FAILING call: the next search runs without options and leaves the poisoned n-best buffers alone
    ra, rc, dec, lp, nbest, nlp = _c_search(m, fr, (N, RP), beams=0)
    assert ra == 0 and rc == ERR_ARG and bool((dec == -777).all())
    _, rc, dec, lp, _, _ = _c_search(m, fr)
    assert rc == 0 and torch.equal(dec, before[0]) and torch.equal(lp[:, None], before[1])
    assert bool((nbest == -777).all()) and bool(torch.isnan(nlp).all())
    # n > beams * per_node_beam_size at the consuming call: refused with nothing launched, consumed all the same
    ra, rc, dec, lp, nbest, nlp = _c_search(m, fr, (9, 1.0))
    assert ra == 0 and rc == ERR_ARG and b"num_keep_best" in lib.gitcap_last_error(h)
    assert bool((dec == -777).all()) and bool((nbest == -777).all())
    _, rc, dec, lp, _, _ = _c_search(m, fr)
    assert rc == 0 and torch.equal(dec, before[0])
    # left pending across gitcap_encode (and a greedy call), consumed by the search behind them
    nbest = torch.full((B, N, L), -777, dtype=torch.int64, device="cuda")
    nlp = torch.full((B, N), float("nan"), device="cuda")
    o = CSearchOptions(N, RP, nbest.data_ptr(), nlp.data_ptr())
    assert lib.gitcap_attach_search_options(h, ctypes.byref(o)) == 0
    assert lib.gitcap_encode(h, ptr(fr), B, F, None, stream()) == 0
    ids = torch.empty((B, L + 1), dtype=torch.int64, device="cuda")
    assert lib.gitcap_greedy(h, ptr(fr), B, F, L, 0, ptr(ids), None, stream()) == 0
    torch.cuda.synchronize()
    assert bool((nbest == -777).all())
    _, rc, dec, lp, _, _ = _c_search(m, fr)
    assert rc == 0 and torch.equal(nbest, dev[0]) and torch.equal(nlp, dev[1]) and torch.equal(dec, dev[0][:, 0])
    # NULL detaches
    nbest.fill_(-777)
    assert lib.gitcap_attach_search_options(h, ctypes.byref(o)) == 0 and lib.gitcap_attach_search_options(h, None) == 0
    _, rc, dec, lp, _, _ = _c_search(m, fr)
    assert rc == 0 and torch.equal(dec, before[0]) and bool((nbest == -777).all())
    # refused values
    for n, rp in ((0, 1.0), (17, 1.0), (-1, 1.0), (2, 0.0), (2, -1.3), (2, float("inf")), (2, float("nan"))):
        bad = CSearchOptions(n, rp, nbest.data_ptr(), nlp.data_ptr())
        assert lib.gitcap_attach_search_options(h, ctypes.byref(bad)) == ERR_ARG, (n, rp)
    assert lib.gitcap_attach_search_options(h, ctypes.byref(CSearchOptions(2, 1.0, None, nlp.data_ptr()))) == ERR_ARG
    assert lib.gitcap_attach_search_options(h, ctypes.byref(CSearchOptions(2, 1.0, nbest.data_ptr(), None))) == ERR_ARG
    assert lib.gitcap_attach_search_options(h, ctypes.byref(CSearchOptions(2, 1.0, nbest.data_ptr() + 4, nlp.data_ptr()))) == ERR_ARG
    assert lib.gitcap_attach_search_options(h, ctypes.byref(CSearchOptions(2, 1.0, nbest.data_ptr(), nlp.data_ptr() + 2))) == ERR_ARG
    assert lib.gitcap_attach_search_options(None, ctypes.byref(o)) == ERR_ARG
    _, rc, dec, lp, _, _ = _c_search(m, fr)                                    # none of them left anything pending
    assert rc == 0 and torch.equal(dec, before[0]) and bool((nbest == -777).all())


def test_batch_invariance_defaults_and_limits(model):
    m, cfg, fr, before, dev, ws0 = model
    for b in range(B):                                                        # a clip alone == the same clip inside the batch
        solo = m.infer(fr[b:b + 1], on_device=True, **KW, **OPT)
        assert torch.equal(solo["predictions"], dev[0][b:b + 1]) and torch.equal(solo["logprobs"], dev[1][b:b + 1])
    r = m.infer(fr, on_device=True, **KW)                                      # a default call after attached ones: what it was before any
    assert torch.equal(r["predictions"], before[0]) and torch.equal(r["logprobs"], before[1])
    assert tuple(r["predictions"].shape) == (B, L) and tuple(r["logprobs"].shape) == (B, 1)
    # the n-best state is workspace: 4 slots x max_batch x 16 x ((max_text_len + 1) ids + score + length), allocated once
    ws = m.workspace_bytes()
    assert ws - ws0 >= 4 * B * 16 * ((L + 1) * 8 + 8)
    m.infer(fr, on_device=True, **KW, **OPT)
    assert m.workspace_bytes() == ws
    for bad in (dict(num_keep_best=9), dict(num_keep_best=0), dict(repetition_penalty=0.0), dict(repetition_penalty=float("nan"))):
        with pytest.raises(ValueError):
            m.infer(fr, on_device=True, **KW, **bad)
        with pytest.raises(ValueError):
            m.infer_async(fr, **KW, **bad)
        with pytest.raises(ValueError):
            m.caption_stream(batch=B, window=F, max_len=L, beam_size=BEAMS, **bad)
    with pytest.raises(ValueError):
        m.caption_stream(batch=B, window=F, max_len=L, num_keep_best=2)        # options of the beam search
    r = m.infer(fr, **KW, num_keep_best=8)                                     # the limit itself: beams * per_node_beam_size
    assert tuple(r["predictions"].shape) == (B, 8, L) and bool((r["logprobs"][:, :N] > -1e4).all())
