"""The forced forms of the token-selection kernels (gitcap_attach_prompt) through their debug hooks, exact equality:
  a. gitcap_dbg_argmax_final_forced (with and without lp, with and without emb) against tests/prompt_reference.py, and bit for bit
     against the unforced kernel run on partials that make the same token win;
  b. gitcap_dbg_beam_step_forced (n = 1, n = 3, sampled) on B = 3 clips (forced, free, done): every field of the state against the
     restatement, untouched fields against their poison.
The inputs are prompt_reference.selection_inputs / beam_inputs; tests/test_prompt.py shows which wrong kernels they catch."""
import ctypes

import numpy as np
import pytest
import torch

import prompt_reference as P
from gpu_support import NAN, assert_tail, beam_state, lib, poisoned, ptr, same_bits, stream, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

LD_OUT, LD_LP = 3, 2


def _run_select(lib, val, idx, psum, step, D, want_lp, prompt=None, lengths=None):
    """One launch of the forced hook (prompt given) or of the plain / _lp hook -> (out [4], sep_cnt [4], lp [4] | None, xf, xb)"""
    rows, nt = val.shape
    d_val, d_idx, d_sum = to_dev(val, torch.float32), to_dev(idx, torch.int32), to_dev(psum, torch.float32)
    out = poisoned((rows + 1) * LD_OUT, -7, torch.int64)
    lp = poisoned((rows + 1) * LD_LP, NAN) if want_lp else None
    sep_cnt = to_dev([100] * (P.SEL_MAX_LEN + 2), torch.int32)      # one counter per step, the step's own is written
    emb = xf = xb = None
    if D:
        from gitcap._lib import CDbgNextEmbed
        g = torch.Generator(device="cuda").manual_seed(D)
        vocab = 16 * nt
        word, pos = torch.randn(vocab, D, device="cuda", generator=g), torch.randn(step + 3, D, device="cuda", generator=g)
        gamma, beta = torch.randn(D, device="cuda", generator=g), torch.randn(D, device="cuda", generator=g)
        xf, xb = poisoned((rows + 1, D), NAN), poisoned((rows + 1, D), NAN, torch.bfloat16)
        emb = CDbgNextEmbed(word.data_ptr(), pos.data_ptr(), gamma.data_ptr(), beta.data_ptr(), 1e-5, D, vocab, step + 1, xf.data_ptr(),
                            xb.data_ptr())
    head = (ptr(d_val), ptr(d_idx), nt, rows, 1, 0, ptr(out), LD_OUT, ptr(sep_cnt), step, P.SEP, ctypes.byref(emb) if emb else None)
    if prompt is not None:
        d_pr, d_len = to_dev(prompt, torch.int64), to_dev(lengths, torch.int32)
        rc = lib.gitcap_dbg_argmax_final_forced(*head, ptr(d_sum) if want_lp else None, ptr(lp), LD_LP, ptr(d_pr), prompt.shape[1], ptr(d_len),
                                                P.SEL_MAX_LEN, stream())
    elif want_lp:
        rc = lib.gitcap_dbg_argmax_final_lp(*head, ptr(d_sum), ptr(lp), LD_LP, stream())
    else:
        rc = lib.gitcap_dbg_argmax_final(*head, stream())
    torch.cuda.synchronize()
    assert rc == 0
    o = out.view(rows + 1, LD_OUT)
    assert bool((o[:, 1:] == -7).all()) and bool((o[rows] == -7).all())
    if want_lp:
        l2 = lp.view(rows + 1, LD_LP)
        assert bool(torch.isnan(l2[:, 1:]).all()) and bool(torch.isnan(l2[rows]).all())
    if D:
        assert bool(torch.isnan(xf[rows]).all()) and bool(torch.isnan(xb[rows].float()).all())
    return o[:rows, 0].clone(), sep_cnt.cpu().tolist(), (lp.view(rows + 1, LD_LP)[:rows, 0].clone() if want_lp else None), xf, xb


@pytest.mark.parametrize("D", [0, 64, 768])
@pytest.mark.parametrize("want_lp", [False, True])
@pytest.mark.parametrize("nt", [9, 257])
def test_argmax_final_forced(lib, nt, want_lp, D):
    val, idx, prompt, lengths = P.selection_inputs(nt)
    rng = np.random.default_rng(nt)
    psum = (rng.random(val.shape) * 3 + 1).astype(np.float32)
    psum[np.isinf(val)] = 0.0
    for step in (P.SEL_STEP - 1, P.SEL_STEP):
        toks, forced, n_sep = P.forced_select(val, idx, prompt, lengths, P.SEL_MAX_LEN, step, P.SEP)
        out, sep, lp, xf, xb = _run_select(lib, val, idx, psum, step, D, want_lp, prompt, lengths)
        assert out.cpu().tolist() == toks
        assert sep == [100 + (n_sep if t == step else 0) for t in range(P.SEL_MAX_LEN + 2)]
        # the unforced kernel on partials that elect the same tokens: out, the embedded rows bit for bit
        val2, idx2 = val.copy(), idx.copy()
        for r, f in enumerate(forced):
            if f:
                val2[r] = np.where(np.isinf(val2[r]), -3.0, val2[r])
                val2[r, toks[r] // 16], idx2[r, toks[r] // 16] = 5.0, toks[r]
        out2, _, _, xf2, xb2 = _run_select(lib, val2, idx2, psum, step, D, False)
        assert torch.equal(out, out2)
        if D:
            assert same_bits(xf[:4], xf2[:4]) and same_bits(xb[:4], xb2[:4])
        if want_lp:                    # free rows: the plain launch's bits on the same partials; forced rows: 0.0f
            _, _, lp0, _, _ = _run_select(lib, val, idx, psum, step, D, True)
            for r, f in enumerate(forced):
                assert (lp[r].view(torch.int32).item() == 0) if f else same_bits(lp[r:r + 1], lp0[r:r + 1]), (r, f)
    # behind the longest prompt the forced hook runs the launch without a prompt: same outputs
    a = _run_select(lib, val, idx, psum, P.SEL_MAX_LEN, D, want_lp, prompt, lengths)
    b = _run_select(lib, val, idx, psum, P.SEL_MAX_LEN, D, want_lp)
    assert torch.equal(a[0], b[0]) and a[1] == b[1]
    # a length beyond max_len is clamped: position max_len - 1 is forced, nothing is read behind the row's max_len columns
    big = np.full(4, 1 << 20, np.int32)
    out, _, _, _, _ = _run_select(lib, val, idx, psum, P.SEL_MAX_LEN - 2, D, want_lp, prompt, big)
    assert out.cpu().tolist() == prompt[:, P.SEL_MAX_LEN - 1].tolist()


def test_forced_hooks_reject_bad_arguments(lib):
    val, idx, prompt, lengths = P.selection_inputs(9)
    d_val, d_idx, d_pr, d_len = to_dev(val, torch.float32), to_dev(idx, torch.int32), to_dev(prompt, torch.int64), to_dev(lengths, torch.int32)
    out = poisoned(4, -7, torch.int64)
    head = (ptr(d_val), ptr(d_idx), 9, 4, 1, 0, ptr(out), 1, None, 2, P.SEP, None, None, None, 0)
    assert lib.gitcap_dbg_argmax_final_forced(*head, None, 8, ptr(d_len), 6, stream()) == -1
    assert lib.gitcap_dbg_argmax_final_forced(*head, ptr(d_pr), 8, None, 6, stream()) == -1
    assert lib.gitcap_dbg_argmax_final_forced(*head, ptr(d_pr), 5, ptr(d_len), 6, stream()) == -1      # ld < max_len
    torch.cuda.synchronize()
    assert bool((out == -7).all())


@pytest.mark.parametrize("n,sampled", [(1, False), (3, False), (3, True)])
@pytest.mark.parametrize("beams", [2, 4])
def test_beam_step_forced(lib, beams, n, sampled):
    st, cs, ci, prompt, lengths, c = P.beam_inputs(beams, n, sampled)
    t, _, bbn = beam_state(c["B"], beams, n, c["L"])
    for k, v in st.items():
        if k != "ids1":                # ids[cur ^ 1] stays poisoned: the step writes columns 0 .. cur_len of it
            t[k].copy_(torch.as_tensor(v).reshape(t[k].shape))
    d_cs = to_dev(cs, torch.float32)
    d_ci = to_dev(np.where(ci == 0x7FFFFFFF, 0x7FFFFFFF, ci), torch.int32)
    d_pr, d_len = to_dev(prompt, torch.int64), to_dev(lengths, torch.int32)
    rc = lib.gitcap_dbg_beam_step_forced(ctypes.byref(bbn), ptr(d_cs), ptr(d_ci), c["B"], beams, c["K"], c["V"], c["cur_len"], c["L"], c["eos"],
                                         ctypes.c_float(c["lp"]), c["cur"], int(sampled), ptr(d_pr), prompt.shape[1], ptr(d_len), c["pmax"],
                                         stream())
    torch.cuda.synchronize()
    assert rc == 0
    want = {k: v.copy() for k, v in st.items()}
    P.beam_step(want, n, cs, ci, c["B"], beams, c["K"], c["V"], c["cur_len"], c["L"], c["eos"], c["lp"], c["cur"], sampled, prompt, lengths,
                c["pmax"])
    for k, v in want.items():
        got = t[k].cpu().numpy().reshape(v.shape)
        if v.dtype == np.float32:
            assert np.allclose(got, v, rtol=1e-6, atol=0), k
        else:
            assert np.array_equal(got, v), (k, got, v)
    # the forced and the done clip: their floats are the bits they were (nothing rewrote them)
    nb = beams
    assert np.array_equal(t["beam_scores"].cpu().numpy()[:nb], st["beam_scores"][:nb])
    assert np.array_equal(t["hyp_score"].cpu().numpy().reshape(c["B"], n)[[0, 2]], st["hyp_score"][[0, 2]])
    # poison: ids[cur ^ 1] behind column cur_len, ids[cur] as it was
    assert bool((t["ids1"][:, c["cur_len"] + 1:] == P.POISON).all())
    assert np.array_equal(t["ids0"].cpu().numpy(), st["ids0"])
    # a prompt as long as max_len leaves no position to decode: refused
    assert lib.gitcap_dbg_beam_step_forced(ctypes.byref(bbn), ptr(d_cs), ptr(d_ci), c["B"], beams, c["K"], c["V"], c["cur_len"], c["L"], c["eos"],
                                           ctypes.c_float(c["lp"]), c["cur"], int(sampled), ptr(d_pr), prompt.shape[1], ptr(d_len), c["L"],
                                           stream()) == -1
