"""Sampling (do_sample) of the device-resident search through the public surface -- gitcap_attach_sampling, infer / infer_async /
caption_stream -- on git_tiny with the seeded weights the fixtures of tests/golden/ were made with.

Reference: the host operator (gitcap/search.py) with torch.multinomial replaced by the contract's draws
(sampling_reference.multinomial_from_philox), replayed on the logits the device search itself saved, step by step.  A clip is left out
from its first undecidable decision on (sampling_reference: margins under their bounds) and counted: at most one clip in ten.

The replay runs on four sets of frames (two sampling seeds x three filters x two clips each: 48 clips) of git_tiny, and once at the
real vocabulary (git_base, 30522 columns)."""
import ctypes

import numpy as np
import pytest
import torch

import sampling_reference as S
from gitcap.config import git_tiny
from gitcap.weights import synthetic_weights
from gpu_support import captioner_cls, ptr, stream  # noqa: F401
from oracle.git_oracle import make_frames

pytestmark = pytest.mark.gpu

ERR_ARG = -1
B, F, BEAMS, PNB, L, LP = 2, 2, 2, 2, 8, 0.6
KW = dict(beam_size=BEAMS, max_steps=L, length_penalty=LP, per_node_beam_size=PNB)
SEEDS = (11, 2 ** 40 + 5)
FRAME_SEEDS = (1247, 1248, 1249, 1250)
FILTERS = (dict(), dict(top_k=5, temperature=0.7), dict(top_p=0.9, temperature=2.0, repetition_penalty=1.3))


@pytest.fixture(scope="module")
def model(captioner_cls):
    cfg = git_tiny(2)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=B, max_frames=F, max_text_len=L, max_beams=4, stop="never")
    fr = make_frames(B, F, cfg.image_size, 1247).cuda()
    r = m.infer(fr, on_device=True, **KW)                  # before any attachment
    return m, cfg, fr, (r["predictions"].clone(), r["logprobs"].clone()), None


def test_device_sampling_vs_replayed_host_operator(model, monkeypatch):
    from gitcap.search import GeneratorWithBeamSearch
    m, cfg, fr, _, _ = model
    V, eos = cfg.vocab_size, cfg.sep_token_id
    clips = dropped = 0
    real_multinomial = torch.multinomial
    for frame_seed, seed, f in [(a, b, c) for a in FRAME_SEEDS for b in SEEDS for c in FILTERS]:
        fr = make_frames(B, F, cfg.image_size, frame_seed).cuda()
        fut = m.infer_async(fr, save_logits=True, do_sample=True, seed=seed, **KW, **f)      # gitcap_beam_search_submit
        r = fut.result()
        assert r["seed"] == seed
        steps = r["logits_dict"].cpu()
        assert tuple(steps.shape) == (L - 1, B * BEAMS, V)
        rp, T = f.get("repetition_penalty", 1.0), f.get("temperature", 1.0)
        top_k, top_p = f.get("top_k", 0), f.get("top_p", 1.0)
        monkeypatch.setattr(torch, "multinomial", S.multinomial_from_philox(seed))
        host = GeneratorWithBeamSearch(eos, L, BEAMS, PNB, LP, repetition_penalty=rp, temperature=T)
        hdec, hlps, _ = host.search(torch.full((B, 1), cfg.cls_token_id), lambda ids: steps[ids.shape[1] - 1], do_sample=True,
                                    top_k=top_k, top_p=top_p)
        monkeypatch.setattr(torch, "multinomial", real_multinomial)
        # decidability, from the restated loop on the same logits
        book = S.Book(B, BEAMS, 1, L, cfg.cls_token_id, eos, LP)
        ok = [True] * B
        for cur_len in range(1, L):
            d = S.draw_rows(steps[cur_len - 1].numpy(), book.beam_scores, book.ids, rp, T, top_k, top_p, seed, cur_len, PNB)
            for row in range(B * BEAMS):
                if not book.done[row // BEAMS] and not all(S.decidable(d, row)):
                    ok[row // BEAMS] = False
            ci, cs = S.layout(d["words"], d["scores"], B, BEAMS, PNB, V)
            book.step(cs.astype(np.float32), ci, V, cur_len)
        for b in range(B):
            clips += 1
            if not ok[b]:
                dropped += 1
                continue
            assert torch.equal(r["predictions"][b].cpu(), hdec[b]), (seed, f, b, r["predictions"][b], hdec[b])
            assert abs(float(r["logprobs"][b, 0]) - float(hlps[b, 0])) <= 1e-4, (seed, f, b)
    print("clips compared %d, dropped as undecidable %d" % (clips, dropped))
    assert dropped * 10 <= clips


@pytest.fixture(scope="module")
def base_model():
    """GIT-base (vocabulary 30522) as tests/test_parity_gpu.py::test_device_beam_search_base_size builds it."""
    from gitcap.config import git_base
    from gitcap.model import GitCaptioner
    cb = git_base(2)
    mb = GitCaptioner(cb, synthetic_weights(cb, 0), max_batch=2, max_frames=2, max_text_len=12, max_beams=4)
    return mb, cb, make_frames(2, 2, cb.image_size, 52).cuda()


def test_sampling_at_the_real_vocabulary(base_model, monkeypatch):
    """V = 30522, beams 4: the device search against the host operator replayed on its logits, and the same bits from infer.  The
    filters are top_k and none: the synthetic weights give flat rows, and on a flat row this wide the cumulative masses around a top_p
    cut lie a few bounds apart (sampling_reference.row_cases), so top_p at this width is tested on rows, not on whole searches."""
    from gitcap.search import GeneratorWithBeamSearch
    mb, cb, fr = base_model
    nb, steps_n = 4, 6
    kw = dict(beam_size=nb, max_steps=steps_n, length_penalty=LP, per_node_beam_size=PNB)
    V, eos = cb.vocab_size, cb.sep_token_id
    assert V == 30522
    clips = dropped = 0
    real_multinomial = torch.multinomial
    for seed, f in [(a, c) for a in (2 ** 33 + 9, 17) for c in (dict(top_k=50), dict(top_k=8, temperature=0.7, repetition_penalty=1.3),
                                                               dict(temperature=1.5))]:
        r = mb.infer_async(fr, save_logits=True, do_sample=True, seed=seed, **kw, **f).result()
        same = mb.infer(fr, do_sample=True, seed=seed, **kw, **f)
        assert torch.equal(same["predictions"], r["predictions"]) and torch.equal(same["logprobs"], r["logprobs"])
        steps = r["logits_dict"].cpu()
        rp, T = f.get("repetition_penalty", 1.0), f.get("temperature", 1.0)
        top_k, top_p = f.get("top_k", 0), f.get("top_p", 1.0)
        monkeypatch.setattr(torch, "multinomial", S.multinomial_from_philox(seed))
        host = GeneratorWithBeamSearch(eos, steps_n, nb, PNB, LP, repetition_penalty=rp, temperature=T)
        hdec, hlps, _ = host.search(torch.full((2, 1), cb.cls_token_id), lambda ids: steps[ids.shape[1] - 1], do_sample=True,
                                    top_k=top_k, top_p=top_p)
        monkeypatch.setattr(torch, "multinomial", real_multinomial)
        book = S.Book(2, nb, 1, steps_n, cb.cls_token_id, eos, LP)
        ok = [True, True]
        for cur_len in range(1, steps_n):
            d = S.draw_rows(steps[cur_len - 1].numpy(), book.beam_scores, book.ids, rp, T, top_k, top_p, seed, cur_len, PNB)
            for row in range(2 * nb):
                if not book.done[row // nb] and not all(S.decidable(d, row)):
                    ok[row // nb] = False
            ci, cs = S.layout(d["words"], d["scores"], 2, nb, PNB, V)
            book.step(cs.astype(np.float32), ci, V, cur_len)
        for b in range(2):
            clips += 1
            if not ok[b]:
                dropped += 1
                print("undecidable:", seed, f, "clip", b)
                continue
            assert torch.equal(r["predictions"][b].cpu(), hdec[b]), (f, b, r["predictions"][b], hdec[b])
            assert abs(float(r["logprobs"][b, 0]) - float(hlps[b, 0])) <= 1e-4, (f, b)
    print("clips compared %d, dropped as undecidable %d" % (clips, dropped))
    assert dropped * 10 <= clips


def test_same_seed_same_bits_through_every_entry_point(model):
    m, cfg, fr, before, _ = model
    opt = dict(do_sample=True, top_k=20, temperature=1.5, seed=99)
    a = m.infer(fr, on_device=True, **KW, **opt)
    assert a["seed"] == 99 and tuple(a["predictions"].shape) == (B, L)
    b = m.infer(fr, **KW, **opt)
    futs = [m.infer_async(fr, **KW, **opt), m.infer_async(fr, **KW), m.infer_async(fr, **KW, **opt)]
    got = [f.result() for f in futs]
    s = m.caption_stream(batch=B, window=F, max_len=L, **{k: v for k, v in KW.items() if k != "max_steps"}, **opt)
    w = s.push(fr)
    assert s.last_seed == 99
    for x in (b, got[0], got[2], w):
        assert torch.equal(x["predictions"], a["predictions"]) and torch.equal(x["logprobs"], a["logprobs"])
    assert torch.equal(got[1]["predictions"], before[0]) and torch.equal(got[1]["logprobs"], before[1]) and "seed" not in got[1]
    # seed=None: one int64 from torch's global CPU generator
    torch.manual_seed(5)
    c = m.infer(fr, **KW, do_sample=True)
    torch.manual_seed(5)
    d = m.infer(fr, **KW, do_sample=True)
    assert c["seed"] == d["seed"] and torch.equal(c["predictions"], d["predictions"])
    # other seeds, other captions (a hot temperature flattens the tiny model's rows)
    caps = {tuple(m.infer(fr, **KW, do_sample=True, temperature=50.0, seed=s_)["predictions"].flatten().tolist()) for s_ in range(4)}
    assert len(caps) > 1
    # the host path draws from another stream but runs, seeded
    h1 = m.infer(fr, on_device=False, **KW, do_sample=True, top_k=20, seed=3)
    h2 = m.infer(fr, on_device=False, **KW, do_sample=True, top_k=20, seed=3)
    assert h1["seed"] == 3 and torch.equal(h1["predictions"], h2["predictions"])


def test_top_k_1_keeps_two_columns(model):
    """min_tokens_to_keep = 2: every step's candidates of a row are its two largest logits, in either order."""
    m, cfg, fr, _, _ = model
    r = m.infer_async(fr, save_logits=True, do_sample=True, top_k=1, seed=7, **KW).result()
    steps = r["logits_dict"]
    book = S.Book(B, BEAMS, 1, L, cfg.cls_token_id, cfg.sep_token_id, LP)
    for cur_len in range(1, L):
        d = S.draw_rows(steps[cur_len - 1].cpu().numpy(), book.beam_scores, book.ids, 1.0, 1.0, 1, 1.0, 7, cur_len, PNB)
        top2 = steps[cur_len - 1].topk(2, dim=-1).indices.cpu()
        for row in range(B * BEAMS):
            assert d["kept"][row] == 2 and sorted(d["words"][row]) == sorted(top2[row].tolist())
        ci, cs = S.layout(d["words"], d["scores"], B, BEAMS, PNB, cfg.vocab_size)
        book.step(cs.astype(np.float32), ci, cfg.vocab_size, cur_len)
    dec, lps = book.finish()
    assert np.array_equal(r["predictions"].cpu().numpy(), dec[:, 0])


def test_nothing_attached_gives_the_recorded_bits(model, base_model):
    """The default search with the sampling code linked in: tests/golden/device_beam_base.npz at the bar tests/test_parity_gpu.py
    holds it to (ids exactly, scores to 1e-3); and on this module's handle, after sampled calls, the bits from before them.
    Sampling allocates nothing: the workspace is the same before and after a sampled call."""
    import os
    m, cfg, fr, before, _ = model
    ws = m.workspace_bytes()
    m.infer(fr, **KW, do_sample=True, seed=1)
    assert m.workspace_bytes() == ws
    r = m.infer(fr, on_device=True, **KW)
    assert torch.equal(r["predictions"], before[0]) and torch.equal(r["logprobs"], before[1])
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "device_beam_base.npz"))
    mb, cb, frb = base_model
    out = mb.infer(frb, beam_size=4, max_steps=10, length_penalty=0.6, on_device=True)
    assert np.array_equal(g["predictions"], out["predictions"].cpu().numpy())
    assert np.allclose(g["logprobs"], out["logprobs"].cpu().numpy().reshape(-1), atol=1e-3)


def test_refusals_consume_the_attachment(model):
    from gitcap._lib import CSamplingOptions
    m, cfg, fr, before, _ = model
    lib, h = m._lib, m._handle

    def search(pnb=PNB, beams=BEAMS):
        dec = torch.full((B, L), -777, dtype=torch.int64, device="cuda")
        lp = torch.full((B,), float("nan"), device="cuda")
        rc = lib.gitcap_beam_search(h, ptr(fr), B, F, beams, L, ctypes.c_float(LP), pnb, ptr(dec), ptr(lp), stream())
        torch.cuda.synchronize()
        return rc, dec, lp

    for bad in ((0.0, 0, 1.0), (float("nan"), 0, 1.0), (float("inf"), 0, 1.0), (1.0, -1, 1.0), (1.0, 0, 0.0), (1.0, 0, 1.01),
                (1.0, 0, float("nan"))):
        assert lib.gitcap_attach_sampling(h, ctypes.byref(CSamplingOptions(bad[0], bad[1], bad[2], 1))) == ERR_ARG, bad
    assert lib.gitcap_attach_sampling(None, ctypes.byref(CSamplingOptions(1.0, 0, 1.0, 1))) == ERR_ARG
    rc, dec, lp = search()                                   # nothing is pending after the refused attaches
    assert rc == 0 and torch.equal(dec, before[0]) and torch.equal(lp[:, None], before[1])
    # per_node_beam_size beyond what the filter is sure to keep: refused at the consuming call, nothing launched, consumed
    for smp, pnb, beams in (((1.0, 0, 0.9), 3, 2), ((1.0, 2, 1.0), 3, 2), ((1.0, 1, 1.0), 4, 2), ((1.0, 3, 1.0), 4, 4)):
        assert lib.gitcap_attach_sampling(h, ctypes.byref(CSamplingOptions(smp[0], smp[1], smp[2], 1))) == 0
        rc, dec, lp = search(pnb, beams)
        assert rc == ERR_ARG and bool((dec == -777).all()) and bool(torch.isnan(lp).all()), (smp, pnb)
        rc, dec, lp = search()
        assert rc == 0 and torch.equal(dec, before[0]) and torch.equal(lp[:, None], before[1]), (smp, pnb)
    # detach
    assert lib.gitcap_attach_sampling(h, ctypes.byref(CSamplingOptions(1.0, 0, 1.0, 1))) == 0 and lib.gitcap_attach_sampling(h, None) == 0
    rc, dec, lp = search()
    assert rc == 0 and torch.equal(dec, before[0])
    # the Python surface refuses with the same messages
    with pytest.raises(ValueError, match="exceeds the columns"):
        m.infer(fr, beam_size=2, max_steps=L, per_node_beam_size=3, do_sample=True, top_p=0.9)
    with pytest.raises(ValueError, match="temperature"):
        m.infer(fr, **KW, do_sample=True, temperature=0.0)
    with pytest.raises(ValueError, match="top_p"):
        m.infer_async(fr, **KW, do_sample=True, top_p=0.0)
    with pytest.raises(ValueError, match="top_k"):
        m.caption_stream(batch=B, window=F, max_len=L, beam_size=BEAMS, do_sample=True, top_k=-2)
