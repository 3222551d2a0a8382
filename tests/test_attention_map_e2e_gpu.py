"""Attention maps through the public surface of the teacher: GitCaptioner.attention, greedy_decode(return_attention=True),
gitcap_attention_map's state errors and the surfaces that refuse -- on git_tiny and the 768-wide mid-size model of gpu_support."""
import numpy as np
import pytest
import torch

from gitcap import _lib
from gitcap.confidence import frame_attribution
from gitcap.config import git_tiny
from gitcap.weights import synthetic_weights
from gpu_support import captioner_cls, mid768, ptr, same_bits, stream  # noqa: F401
from oracle.git_oracle import make_frames
from text_rows_reference import U32

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_STATE = -1, -2
MAX_LEN = 7


def row_sum_bound(cfg, fr, ids):
    """sum_f frame_mass + text_mass against 1, per (row, position): the sum of the row's element bounds of
    tests/attention_map_reference.py, evaluated on the q and k of the oracle's bf16-emulating pass over the same frames and ids
    (the model's own magnitudes), doubled because the device's q and k are those only up to bf16 rounding of the stack."""
    import attention_map_reference as R
    case = R.case_from_oracle(cfg, synthetic_weights(cfg, 0), fr.cpu(), ids.cpu())
    _, _, _, bf, bt, _ = R.maps_fp64(case, want_bound=True)
    return 2.0 * (bf.sum(-1) + bt)


@pytest.fixture(scope="module", params=["tiny", "mid768"])
def teacher(request, captioner_cls):
    cfg = git_tiny(3) if request.param == "tiny" else mid768()
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=2, max_frames=3, max_text_len=MAX_LEN + 1, max_beams=3, stop="never")
    fr = make_frames(2, 3, cfg.image_size, 1234).cuda()
    return m, cfg, fr


def test_greedy_attention_is_attention_of_the_result(teacher):
    m, cfg, fr = teacher
    ids0, lp0 = m.greedy_decode(fr, max_len=MAX_LEN, return_logprobs=True)
    ids, lp, fa, ta = m.greedy_decode(fr, max_len=MAX_LEN, return_logprobs=True, return_attention=True)
    assert torch.equal(ids, ids0) and same_bits(lp, lp0)
    assert fa.shape == (2, MAX_LEN, 3) and ta.shape == (2, MAX_LEN)
    d = m.attention(fr, ids, until_sep=False, patches=True)
    assert same_bits(d["frame_attention"], fa) and same_bits(d["text_attention"], ta)
    N = (cfg.image_size // cfg.patch_size) ** 2 + 1
    assert d["patch_attention"].shape == (2, MAX_LEN, 3, N)
    total = fa.double().sum(-1) + ta.double()
    bound = row_sum_bound(cfg, fr, ids[:, :-1])
    err = (total - 1).abs().cpu().numpy()
    print(f"rows sum to 1 within {err.max():.3e} (bound {bound.min():.3e} .. {bound.max():.3e})")
    assert (err <= bound).all()
    # the frame's mass is the sum of its patch row, up to the fp32 additions
    assert float((d["patch_attention"].double().sum(-1) - fa.double()).abs().max()) <= (N + 8) * U32
    assert bool((ta[:, 0] < 1).all()) and bool((fa > 0).all())
    # one layer at a time averages to all layers
    per = torch.stack([m.attention(fr, ids, until_sep=False, layer=l)["frame_attention"].double() for l in range(cfg.dec_layers)]).mean(0)
    assert float((per - fa.double()).abs().max()) <= 4 * U32
    a = frame_attribution(d)
    assert a["frame"].shape == (2, MAX_LEN) and torch.equal(a["frame"], fa.argmax(-1)) and a["mean_mass"].shape == (2, 3)
    assert float((a["image_share"].double() - (1 - ta.double()).mean(-1)).abs().max()) <= 1e-5


def test_lengths_and_until_sep_zero_the_tail(teacher):
    m, cfg, fr = teacher
    ids = m.greedy_decode(fr, max_len=MAX_LEN)
    full = m.attention(fr, ids, until_sep=False)
    cut = m.attention(fr, ids, until_sep=False, lengths=torch.tensor([3, 1]))
    assert same_bits(cut["frame_attention"][0, :2].contiguous(), full["frame_attention"][0, :2].contiguous())
    assert bool((cut["frame_attention"][0, 2:] == 0).all()) and bool((cut["text_attention"][0, 2:] == 0).all())
    assert bool((cut["frame_attention"][1] == 0).all()) and bool((cut["text_attention"][1] == 0).all())
    y = ids.clone()
    y[0, 2] = cfg.sep_token_id
    y[1, 1:] += (y[1, 1:] == cfg.sep_token_id).long()
    sep = m.attention(fr, y)
    assert bool((sep["text_attention"][0, :2] > 0).all()) and bool((sep["text_attention"][0, 2:] == 0).all())
    assert bool((sep["text_attention"][1] > 0).all())
    assert frame_attribution(sep)["frame"][0, 2:].tolist() == [-1] * (MAX_LEN - 2)


def test_ragged_clip_equals_the_clip_alone(teacher):
    m, cfg, fr = teacher
    clips = [fr[0, :1].contiguous(), fr[1].contiguous()]
    ids, fa, ta = m.greedy_decode(clips, max_len=MAX_LEN, return_attention=True)
    assert fa.shape == (2, MAX_LEN, 3) and bool((fa[0, :, 1:] == 0).all()) and bool((fa[0, :, 0] > 0).all())
    d = m.attention(clips, ids, until_sep=False, patches=True)
    assert same_bits(d["frame_attention"], fa) and same_bits(d["text_attention"], ta)
    N = d["patch_attention"].shape[-1]
    assert bool((d["patch_attention"][0, :, 1:] == 0).all())
    for b in range(2):
        alone = m.attention(clips[b][None], ids[b:b + 1], until_sep=False, patches=True)
        F = clips[b].shape[0]
        assert same_bits(alone["frame_attention"], fa[b:b + 1, :, :F].contiguous())
        assert same_bits(alone["text_attention"], ta[b:b + 1].contiguous())
        assert same_bits(alone["patch_attention"], d["patch_attention"][b:b + 1, :, :F].contiguous())


def test_candidates_map_to_their_clip(teacher):
    m, cfg, fr = teacher
    g = torch.Generator().manual_seed(5)
    y = torch.randint(0, cfg.vocab_size, (2, 3, 5), generator=g).cuda()
    y[..., 0] = cfg.cls_token_id
    y[y == cfg.sep_token_id] += 1
    d = m.attention(fr, y, until_sep=False)
    assert d["frame_attention"].shape == (2, 3, 4, 3) and d["text_attention"].shape == (2, 3, 4)
    for i in range(3):
        one = m.attention(fr, y[:, i].contiguous(), until_sep=False)
        assert same_bits(one["frame_attention"], d["frame_attention"][:, i].contiguous())
        assert same_bits(one["text_attention"], d["text_attention"][:, i].contiguous())


def test_state_errors_are_messages(captioner_cls):
    cfg = git_tiny(2)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=2, max_frames=2, max_text_len=MAX_LEN + 1, max_beams=3, stop="never")
    fr = make_frames(2, 2, cfg.image_size, 7).cuda()
    fm, tm = torch.zeros(2, MAX_LEN, 2, device="cuda"), torch.zeros(2, MAX_LEN, device="cuda")

    def ask(rows=2, T=MAX_LEN, layer=-1):
        rc = m._lib.gitcap_attention_map(m._handle, rows, T, layer, None, ptr(fm), 2, ptr(tm), None, 0, stream())
        return rc, m._lib.gitcap_last_error(m._handle).decode()
    rc, msg = ask()
    assert rc == ERR_STATE and "no synchronous text pass" in msg            # nothing has run
    m.forward_image_enc(fr)
    assert ask()[0] == ERR_STATE                                            # an image pass alone fills no text cache
    ids = m.greedy_decode(fr, max_len=4)
    assert ask(T=4)[0] == 0
    rc, msg = ask(T=5)
    assert rc == ERR_STATE and "exceeds the positions" in msg
    assert ask(rows=1, T=4)[0] == ERR_ARG and ask(T=4, layer=cfg.dec_layers)[0] == ERR_ARG
    m.infer(fr, beam_size=2, max_steps=4, on_device=True)
    rc, msg = ask(T=2)
    assert rc == ERR_STATE and "beam search" in msg
    torch.cuda.synchronize()
    d = m.attention(fr, ids, until_sep=False)                               # beam callers: attention(x, predictions)
    assert d["frame_attention"].shape == (2, 4, 2)
    with pytest.raises(ValueError, match="return_attention"):
        m.greedy_decode(fr, max_len=4, draft=ids, return_attention=True)
    for call in (lambda: m.greedy_decode_async(fr, max_len=4, return_attention=True),
                 lambda: m.infer(fr, beam_size=2, max_steps=4, return_attention=True),
                 lambda: m.infer_async(fr, beam_size=2, max_steps=4, return_attention=True),
                 lambda: m.caption_stream(batch=1, max_len=4, return_attention=True)):
        with pytest.raises(ValueError, match=r"return_attention= is not taken by .*attention\(x, predictions\)"):
            call()


def test_more_clips_than_max_batch_go_through_in_chunks(teacher):
    """B = 3 on a handle of max_batch = 2: two chunks, dense and ragged (the second chunk's one-frame clip is padded to the widest)"""
    m, cfg, fr = teacher
    fr3 = torch.cat([fr, fr[:1].flip(1)], 0).contiguous()
    ids, fa, ta = m.greedy_decode(fr3, max_len=4, return_attention=True)
    d = m.attention(fr3, ids, until_sep=False)
    assert fa.shape == (3, 4, 3) and same_bits(d["frame_attention"], fa) and same_bits(d["text_attention"], ta)
    for b in range(3):
        one = m.attention(fr3[b:b + 1], ids[b:b + 1], until_sep=False)
        assert same_bits(one["frame_attention"], fa[b:b + 1].contiguous()) and same_bits(one["text_attention"], ta[b:b + 1].contiguous())
    clips = [fr[0].contiguous(), fr[1, :2].contiguous(), fr[0, :1].contiguous()]
    ids, fa, ta = m.greedy_decode(clips, max_len=4, return_attention=True)
    d = m.attention(clips, ids, until_sep=False, patches=True)
    assert fa.shape == (3, 4, 3) and same_bits(d["frame_attention"], fa) and same_bits(d["text_attention"], ta)
    assert bool((fa[1, :, 2:] == 0).all()) and bool((fa[2, :, 1:] == 0).all()) and bool((d["patch_attention"][2, :, 1:] == 0).all())
    for b in range(3):
        one = m.attention(clips[b][None], ids[b:b + 1], until_sep=False)
        F = clips[b].shape[0]
        assert same_bits(one["frame_attention"], fa[b:b + 1, :, :F].contiguous()) and same_bits(one["text_attention"], ta[b:b + 1].contiguous())


# ---- student --------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=["tiny", "base"])
def student(request):
    from gpu_support import make_student, student_cfg
    from oracle.student_oracle import make_memory
    cfg = student_cfg(request.param)
    m = make_student(request.param, max_batch=4, max_text_len=MAX_LEN, stop="never")
    return m, cfg, make_memory(2, cfg.mem_tokens, cfg.d_model, 5).cuda()


def test_student_greedy_attention_is_attention_of_the_result(student):
    m, cfg, mem = student
    ids0, lp0 = m.greedy_decode(mem, max_len=MAX_LEN, return_logprobs=True)
    ids, lp, fa = m.greedy_decode(mem, max_len=MAX_LEN, return_logprobs=True, return_attention=True)
    assert torch.equal(ids, ids0) and same_bits(lp, lp0) and fa.shape == (2, MAX_LEN, cfg.mem_tokens)
    d = m.attention(mem, ids, until_sep=False)
    assert same_bits(d["frame_attention"], fa)
    # every position's frames sum to 1: H x L probabilities of sum 1 +- gamma(6) + u each, their mean, F fp32 values added in fp64
    assert float((fa.double().sum(-1) - 1).abs().max()) <= (6 + 2 + cfg.n_head * cfg.num_decoder_layers + 1 + cfg.mem_tokens) * U32
    per = torch.stack([m.attention(mem, ids, until_sep=False, layer=l)["frame_attention"].double() for l in range(cfg.num_decoder_layers)]).mean(0)
    assert float((per - fa.double()).abs().max()) <= 4 * U32
    for b in range(2):          # a row alone
        assert same_bits(m.attention(mem[b:b + 1], ids[b:b + 1], until_sep=False)["frame_attention"], fa[b:b + 1].contiguous())
    cut = m.attention(mem, ids, until_sep=False, lengths=torch.tensor([3, 1]))["frame_attention"]
    assert same_bits(cut[0, :2].contiguous(), fa[0, :2].contiguous()) and bool((cut[0, 2:] == 0).all()) and bool((cut[1] == 0).all())
    y = torch.stack([ids, ids.flip(1)], 1).contiguous()
    y[:, 1, 0] = cfg.cls_token_id
    c = m.attention(mem, y, until_sep=False)["frame_attention"]
    assert c.shape == (2, 2, MAX_LEN, cfg.mem_tokens) and same_bits(c[:, 0].contiguous(), fa)
    assert frame_attribution(fa)["frame"].shape == (2, MAX_LEN)
    ids2 = m.greedy_decode(mem, max_len=MAX_LEN)                      # the plain call after it is the plain call
    assert torch.equal(ids2, ids0)
    for call in (lambda: m.beam_search(mem, max_len=4, k=2, return_attention=True), lambda: m.caption_stream(return_attention=True)):
        with pytest.raises(ValueError, match="return_attention= is not taken by"):
            call()
