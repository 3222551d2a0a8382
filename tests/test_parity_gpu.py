"""Parity of the HIP path (through the C ABI) against the CPU oracle and the committed HF-generated
golden vectors.  Run on the MI355X box:  python -m pytest tests -m gpu -x -q

Numerics contract (DESIGN.md par. 3): GEMM operands are bf16 (weights, the activations fed to a
GEMM, q/k/v, softmax probabilities, GELU outputs); accumulators, residual stream, LayerNorm,
softmax statistics, embeddings and logits are fp32.  Tolerances below are stated against
  (a) the oracle run with the SAME rounding points (emulate_bf16=True): differences come only from
      summation order / exp implementation, amplified where a value sits on a bf16 rounding boundary;
  (b) the fp32 oracle: the device must not be further from fp32 than (a) is, within a factor.
Token parity is asserted token-for-token wherever the oracle's top-1/top-2 margin exceeds the
logit tolerance; inside a near-tie either candidate is accepted and the comparison of that row
stops (a different token legitimately changes everything after it).
"""
import os
import pickle

import numpy as np
import pytest
import torch

from gitcap.config import git_base, git_tiny
from gitcap.weights import quantize_weights_fp8, synthetic_weights
from oracle.git_oracle import GitOracle, make_frames
from gpu_support import captioner_cls, ptr  # noqa: F401

pytestmark = pytest.mark.gpu

LOGIT_TOL_EMUL = 0.08      # |dev - bf16-emulating oracle| on logits with std ~4  (2 % of the spread)
LOGIT_TOL_FP32 = 0.20      # |dev - fp32 oracle|
NEAR_TIE = 0.16            # = 2 x LOGIT_TOL_EMUL: a device token may differ from the oracle's argmax only inside this margin


def _tokens_match_margin_gated(dev_ids, oracle: GitOracle, frames):
    """Teacher-force the oracle on the device's own tokens: every device choice must be the oracle's
    argmax, or lie within NEAR_TIE of it.  Returns the fraction of exact-argmax agreements."""
    logits, _ = oracle.forward_output_logits(frames, dev_ids[:, :-1])
    chosen = logits.gather(2, dev_ids[:, 1:, None]).squeeze(-1)
    gap = logits.max(-1).values - chosen
    assert float(gap.max()) < NEAR_TIE, f"device token outside a near-tie of the oracle: gap {gap.max():.3f}"
    return float((gap == 0).float().mean())


@pytest.mark.parametrize("F", [2, 0])
def test_tiny_stages_vs_oracle(captioner_cls, golden_dir, F):
    cfg = git_tiny(F)
    w = synthetic_weights(cfg, 0)
    g = np.load(os.path.join(golden_dir, f"hf_tiny_F{F}.npz"))
    fr = make_frames(2, max(1, F), cfg.image_size, 1234)
    m = captioner_cls(cfg, w, max_batch=4, max_text_len=16)
    emul, fp32 = GitOracle(cfg, w, emulate_bf16=True), GitOracle(cfg, w)

    _, vis = m.forward_image_enc(fr)
    vis = vis.cpu()
    v_e, v_f = emul.encode_frames(fr), fp32.encode_frames(fr)
    assert (vis - v_e).abs().max() < 2e-2                      # values are O(1..4)
    assert (vis - v_f).abs().max() < 1.5 * (v_e - v_f).abs().max() + 1e-2
    assert np.abs(vis.numpy() - g["visual"]).max() < 0.08      # against the HF fp32 fixture

    ids = torch.from_numpy(g["prefix_ids"])
    lg = m(fr, ids).cpu()
    l_e, _ = emul.forward_output_logits(fr, ids)
    l_f, _ = fp32.forward_output_logits(fr, ids)
    assert (lg - l_e).abs().max() < LOGIT_TOL_EMUL
    assert (lg - l_f).abs().max() < LOGIT_TOL_FP32
    assert np.abs(lg.numpy() - g["logits"]).max() < LOGIT_TOL_FP32      # HF fp32 fixture

    out = m.greedy_decode(fr, max_len=8, stop="never").cpu()
    assert out.shape == (2, 9) and bool((out[:, 0] == cfg.cls_token_id).all())
    frac = _tokens_match_margin_gated(out, emul, fr)
    assert frac >= 0.9
    # golden ids from HF: identical unless a near-tie was hit
    gold = torch.from_numpy(g["greedy_ids"])
    margin = torch.from_numpy(g["greedy_top_vals"][..., 0] - g["greedy_top_vals"][..., 1])
    for b in range(2):
        for t in range(8):
            if out[b, t + 1] != gold[b, t + 1]:
                assert margin[b, t] < NEAR_TIE, (b, t, float(margin[b, t]))
                break


@pytest.mark.parametrize("F,name", [(6, "hf_base_F6.npz"), (0, "hf_base_F1.npz")])
def test_base_vs_hf_golden(captioner_cls, golden_dir, F, name):
    """GIT-base, B=2, 20 greedy tokens, against the HF fp32 run of the same seeded weights/frames."""
    cfg = git_base(F)
    w = synthetic_weights(cfg, 0)
    g = np.load(os.path.join(golden_dir, name))
    fr = make_frames(2, max(1, F), cfg.image_size, int(g["frame_seed"]))
    m = captioner_cls(cfg, w, max_batch=2, max_text_len=24)
    gold = torch.from_numpy(g["greedy_ids"])
    top_i, top_v = torch.from_numpy(g["greedy_top_ids"]), torch.from_numpy(g["greedy_top_vals"])

    _, vis = m.forward_image_enc(fr)
    assert np.abs(vis.cpu()[:, ::97, :32].numpy() - g["visual_slice"]).max() < 0.1   # |values| up to ~3.7
    # teacher-forced on the golden ids: the top-8 logits of each of the 20 steps
    lg = m.forward_decoder(gold[:, :-1], vis).cpu()
    d = (torch.gather(lg, 2, top_i) - top_v).abs()
    assert d.max() < LOGIT_TOL_FP32 and d.mean() < 0.05
    margin = top_v[..., 0] - top_v[..., 1]
    agree = lg.argmax(-1) == gold[:, 1:]
    assert bool(agree[margin > NEAR_TIE].all())

    out = m.greedy_decode(fr, max_len=20, stop="never").cpu()
    for b in range(2):
        for t in range(20):
            if out[b, t + 1] != gold[b, t + 1]:
                assert margin[b, t] < NEAR_TIE, (b, t, float(margin[b, t]))
                break
    if F == 6:      # on this fixture every margin is comfortable: token-for-token
        assert torch.equal(out, gold)


@pytest.mark.parametrize("B,F", [(16, 6), (32, 1)])
def test_full_size_properties(captioner_cls, B, F):
    """BASELINE configs[2] size (16 clips x 6 frames, GIT-base, 20 tokens) and configs[1] size (batch 32, single
    frame): properties that need no CPU run of that size."""
    cfg = git_base(F if F > 1 else 0)
    w = synthetic_weights(cfg, 0)
    m = captioner_cls(cfg, w, max_batch=B, max_frames=F, max_text_len=20)
    fr = make_frames(B, F, cfg.image_size, 99).cuda()
    a = m.greedy_decode(fr, max_len=20, stop="never")
    b = m.greedy_decode(fr, max_len=20, stop="never")
    assert a.shape == (B, 21) and torch.equal(a, b)                      # deterministic (no atomics in the data path)
    assert bool((a[:, 0] == cfg.cls_token_id).all()) and int(a.min()) >= 0 and int(a.max()) < cfg.vocab_size
    # batch invariance: a clip decoded alone gives the same ids as inside the batch
    solo = m.greedy_decode(fr[5:6], max_len=20, stop="never")
    assert torch.equal(solo[0], a[5])
    # chunking over max_batch is transparent
    m4 = captioner_cls(cfg, w, max_batch=4, max_frames=F, max_text_len=20)
    assert torch.equal(m4.greedy_decode(fr[:8], max_len=20, stop="never"), a[:8])
    # KV-cached stepping == one teacher-forced pass over the same tokens, BITWISE (same per-row arithmetic: the
    # argmax of the teacher-forced logits is the cached loop's token at every position of every row)
    _, vis = m.forward_image_enc(fr)
    tf = m.forward_decoder(a[:, :-1], vis)
    assert torch.equal(tf.argmax(-1), a[:, 1:])
    step = m.step_logits(a[:, 7], 7)           # (the image K/V of `fr` are still in the handle) one cached step at position 7
    assert torch.equal(step, tf[:, 7])
    # the oracle on ONE clip of the batch (CPU, seconds): margin-gated token parity at full model size
    emul = GitOracle(cfg, w, emulate_bf16=True)
    _tokens_match_margin_gated(a[5:6].cpu(), emul, fr[5:6].cpu())


@pytest.mark.parametrize("size", ["tiny", "base"])
@pytest.mark.parametrize("B", [1, 2])
def test_one_and_two_row_steps_equal_teacher_forced(captioner_cls, size, B):
    """With one or two text rows the q|k|v launch computes its own input rows (row prologue, csrc/skinny.hip) instead of
    reading what the row kernels wrote; a teacher-forced pass over the same tokens has B*T > 2 rows and uses the row
    kernels.  Same inline code on both paths: every cached step's logits must equal the teacher-forced logits BITWISE,
    and a clip decoded alone (prologue) must give the ids it gets inside a batch of 5 (row kernels)."""
    cfg = git_tiny(2) if size == "tiny" else git_base(2)
    w = synthetic_weights(cfg, 3)
    m = captioner_cls(cfg, w, max_batch=5, max_frames=2, max_text_len=12)
    fr = make_frames(5, 2, cfg.image_size, 17).cuda()
    full = m.greedy_decode(fr, max_len=12, stop="never")
    ids = m.greedy_decode(fr[:B], max_len=12, stop="never")
    assert torch.equal(ids, full[:B])
    _, vis = m.forward_image_enc(fr[:B])
    tf = m.forward_decoder(ids[:, :-1], vis)                       # [B, 12, V], row kernels (B*12 rows)
    assert torch.equal(tf.argmax(-1), ids[:, 1:])
    for t in range(12):                                             # cached single steps, in order (step t writes the K/V of position t)
        step = m.step_logits(ids[:, t], t)
        assert torch.equal(step, tf[:, t]), t


def test_results_do_not_depend_on_speed_switches(captioner_cls):
    """Tile choice (256 x 256 / 128 / 64), the GEMM + LayerNorm epilogue and the one/two-row prologue are speed decisions taken from
    the batch size: flipping each of them at run time (gitcap_dbg_config) must not change a bit of the visual features, the
    teacher-forced logits or the captions -- at GIT-base size, for a batch of 8 clips (256-tile kernels) and a single clip."""
    from gitcap import _lib
    lib = _lib.load()
    cfg = git_base(6)
    w = synthetic_weights(cfg, 0)
    m = captioner_cls(cfg, w, max_batch=8, max_frames=6, max_text_len=12)
    fr = make_frames(8, 6, cfg.image_size, 23).cuda()

    def run(n):
        _, vis = m.forward_image_enc(fr[:n])
        ids = m.greedy_decode(fr[:n], max_len=12, stop="never")
        return vis.clone(), ids.clone(), m.forward_decoder(ids[:, :-1], vis).clone()
    base8, base1 = run(8), run(1)
    assert torch.equal(base1[1], base8[1][:1]) and torch.equal(base1[0], base8[0][:1])
    settings = [(0, 0), (1, 0), (2, 1 << 30), (3, 0), (3, 1 << 30), (2, 1), (5, 0), (7, 0), (10, 0), (11, 0)]   # (key, value); (2, 1): 256-tile kernels even for one clip; (5, 0): every token step embeds its own input rows; (7, 0): FC1 and FC2 of the text rows as two launches; (10, 0): the vocabulary head as one single-wave workgroup per tile; (11, 0): the one/two-row prologue's slab reduce in one wave
    for key, value in settings:
        old = lib.gitcap_dbg_config(key, value)
        assert old >= 0
        try:
            for base, n in ((base8, 8), (base1, 1)):
                got = run(n)
                for a, b in zip(base, got):
                    assert torch.equal(a, b), (key, value, n)
        finally:
            lib.gitcap_dbg_config(key, old)
    # key 8 acts when the weights are finalised: a handle whose text kernels read the row-major weights (no fragment-major
    # copies; its FFN then runs as two launches) gives the same bits
    old = lib.gitcap_dbg_config(8, 0)
    try:
        m2 = captioner_cls(cfg, w, max_batch=8, max_frames=6, max_text_len=12)
    finally:
        lib.gitcap_dbg_config(8, old)
    for base, n in ((base8, 8), (base1, 1)):
        _, vis = m2.forward_image_enc(fr[:n])
        ids = m2.greedy_decode(fr[:n], max_len=12, stop="never")
        assert torch.equal(ids, base[1]) and torch.equal(m2.forward_decoder(ids[:, :-1], vis), base[2]), n
    # key 9: text-attention launches of more (row, head) units than CUs run 8-wave workgroups, two per CU -- 24 single frames are
    # 288 units per token step, their 12-position teacher-forced pass 3456; both forms deal the keys to the same 16 virtual waves
    # (in three handles: fragment-major bf16 weights, e4m3-stored weights, row-major bf16 weights -- the three ways the kernel
    # fetches its output-dense fragments)
    cfg1 = git_base(0)
    w1 = synthetic_weights(cfg1, 0)
    fr1 = make_frames(24, 1, cfg1.image_size, 29).cuda()
    for variant in ("packed", "e4m3", "row-major"):
        old8 = lib.gitcap_dbg_config(8, 0) if variant == "row-major" else None
        try:
            if variant == "e4m3":
                m1 = captioner_cls(cfg1, quantize_weights_fp8(w1), max_batch=24, max_frames=1, max_text_len=12, weight_dtype="fp8_e4m3")
            else:
                m1 = captioner_cls(cfg1, w1, max_batch=24, max_frames=1, max_text_len=12)
        finally:
            if old8 is not None:
                lib.gitcap_dbg_config(8, old8)

        def run1():
            _, vis = m1.forward_image_enc(fr1)
            ids = m1.greedy_decode(fr1, max_len=12, stop="never")
            return ids.clone(), m1.forward_decoder(ids[:, :-1], vis).clone()
        base = run1()
        old = lib.gitcap_dbg_config(9, 0)
        assert old == 1
        try:
            got = run1()
        finally:
            lib.gitcap_dbg_config(9, old)
        assert torch.equal(got[0], base[0]) and torch.equal(got[1], base[1]), variant
        del m1
    assert lib.gitcap_dbg_config(99, 0) < 0


def test_layernorm_exchange_fails_soft(captioner_cls):
    """A fused GEMM + LayerNorm workgroup that gives up waiting for its siblings must not trap: it raises a host-visible
    flag (include/gitcap.h: gitcap_poll_errors).  Forced here with a one-poll spin limit (gitcap_dbg_config(6, 1)): the
    flagged results are undefined, the next check reports GITCAP_ERR_EXCHANGE once, the handle carries on with unfused
    launches (bitwise the same captions), and a CPU-in / CPU-out call repeats itself without the caller noticing."""
    from gitcap import _lib
    lib = _lib.load()
    cfg = git_base(6)
    w = synthetic_weights(cfg, 0)
    fr = make_frames(10, 6, cfg.image_size, 23)               # 11 820 image rows: fused epilogues on 256-row tiles
    m = captioner_cls(cfg, w, max_batch=10, max_frames=6, max_text_len=8)
    want = m.greedy_decode(fr.cuda(), max_len=8, stop="never").cpu()
    m.poll_errors()                                            # healthy
    old = lib.gitcap_dbg_config(6, 1)
    assert old == 0
    try:
        m.greedy_decode(fr.cuda(), max_len=8, stop="never")   # tiles give up after one poll: flag raised, output undefined
        torch.cuda.synchronize()
        with pytest.raises(_lib.GitcapExchangeTimeout, match="timed out"):
            m.poll_errors()
        m.poll_errors()                                        # reported once; the handle is on the unfused launches now
        assert torch.equal(m.greedy_decode(fr.cuda(), max_len=8, stop="never").cpu(), want)
        m.poll_errors()
        # a fresh handle, CPU tensor in -> CPU ids out: the wrapper vouches for the result and re-runs by itself
        m2 = captioner_cls(cfg, w, max_batch=10, max_frames=6, max_text_len=8)
        assert torch.equal(m2.greedy_decode(fr, max_len=8, stop="never"), want)
        with pytest.raises(_lib.GitcapExchangeTimeout):        # entry points refuse once, too (a third handle)
            m3 = captioner_cls(cfg, w, max_batch=10, max_frames=6, max_text_len=8)
            m3.greedy_decode(fr.cuda(), max_len=8, stop="never")
            torch.cuda.synchronize()
            m3.forward_image_enc(fr.cuda())
    finally:
        lib.gitcap_dbg_config(6, old)
    # back on the default limit nothing gives up
    m4 = captioner_cls(cfg, w, max_batch=10, max_frames=6, max_text_len=8)
    assert torch.equal(m4.greedy_decode(fr, max_len=8, stop="never"), want)
    m4.poll_errors()


def test_stop_rule_and_row_semantics(captioner_cls):
    """model.py:184: stop only when ALL rows emit SEP in the same step."""
    cfg = git_tiny(2)
    w = synthetic_weights(cfg, 0)
    w["head.b"] = w["head.b"].copy()
    w["head.b"][cfg.sep_token_id] = 1e4
    m = captioner_cls(cfg, w, max_batch=4, max_text_len=8)
    fr = make_frames(3, 2, cfg.image_size, 1)
    ids = m.greedy_decode(fr, max_len=8)                      # default stop='all_sep'
    assert ids.shape == (3, 2) and bool((ids[:, 1] == cfg.sep_token_id).all())
    assert ids.device == fr.device                            # CPU in, CPU out (real_time_inference.py:57-59)
    full = m.greedy_decode(fr, max_len=8, stop="never")
    assert full.shape == (3, 9)
    # one and two rows (the row-prologue form of the token loop): the same stop rule and tokens
    for n in (1, 2):
        a = m.greedy_decode(fr[:n], max_len=8)
        assert a.shape == (n, 2) and torch.equal(a, ids[:n])
        assert torch.equal(m.greedy_decode(fr[:n], max_len=8, stop="never"), full[:n])
    # without the planted bias rows do not all hit SEP: runs to max_len like the reference loop
    m2 = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=4, max_text_len=8)
    assert m2.greedy_decode(fr, max_len=8).shape == (3, 9)


def test_input_forms_and_edge_cases(captioner_cls):
    cfg = git_tiny(2)
    w = synthetic_weights(cfg, 0)
    m = captioner_cls(cfg, w, max_batch=4, max_text_len=8)
    emul = GitOracle(cfg, w, emulate_bf16=True)
    fr = make_frames(1, 1, cfg.image_size, 3)                # B=1, ragged F=1 < num_frames=2
    out = m.greedy_decode(fr, max_len=4, stop="never").cpu()
    _tokens_match_margin_gated(out, emul, fr)
    img = fr[:, 0]                                            # 4-D single image [B,3,H,W]
    assert torch.equal(m.greedy_decode(img, max_len=4, stop="never").cpu(), out)
    # generate is the alias BASELINE.json names
    assert torch.equal(m.generate(fr, max_len=4, stop="never").cpu(), out)
    # forward_decoder honours a caller-supplied memory tensor (gitcap_set_visual path)
    fr2 = make_frames(2, 2, cfg.image_size, 4)
    _, mem = m.forward_image_enc(fr2)
    y = torch.tensor([[101, 7, 9], [101, 3, 150]])
    a = m.forward_decoder(y, mem)
    b = m.forward_decoder(y, mem.clone())
    assert torch.equal(a, b)
    lists = m.forward_output_logits(fr2, y)                  # teacher API shape (model.py:747-760)
    assert len(lists[0]) == 2 and lists[0][0].shape == (1, 3, cfg.vocab_size)
    assert lists[1][0].shape == (1, 2 * cfg.tokens_per_frame, cfg.enc_width)
    assert torch.allclose(torch.cat(lists[0]), a)


def test_errors_are_loud(captioner_cls):
    from gitcap._lib import GitcapError
    cfg = git_tiny(2)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=2, max_text_len=4)
    with pytest.raises(GitcapError):                          # text before any image
        m.step_logits(torch.tensor([101, 101]), 0)
    with pytest.raises(ValueError):
        m.greedy_decode(make_frames(1, 2, cfg.image_size, 0), max_len=5)          # > max_text_len
    with pytest.raises(ValueError):
        m.forward_image_enc(make_frames(3, 2, cfg.image_size, 0))                 # > max_batch
    with pytest.raises(ValueError):
        m.greedy_decode(torch.zeros(1, 2, 3, 16, 16), max_len=2)                  # wrong image size
    with pytest.raises(GitcapError):
        m.to("cpu")
    bare = captioner_cls(cfg, None, max_batch=1, max_text_len=4)
    with pytest.raises(GitcapError):                          # weights never loaded
        bare.greedy_decode(make_frames(1, 2, cfg.image_size, 0), max_len=2)
    # round-2 entry points: call order and arguments are checked, nothing fails silently
    with pytest.raises(GitcapError, match="before the first"):          # storage must be chosen before any tensor is loaded
        m._call("gitcap_set_weight_storage", 1)
    buf = torch.empty(64, device="cuda")
    with pytest.raises(GitcapError, match="enable"):                    # hidden states were never requested
        m._call("gitcap_hidden_states_read", 1, 2 * cfg.tokens_per_frame, 3, ptr(buf), m._stream())
    with pytest.raises(ValueError):                                     # the device search refuses a beam underflow set-up
        captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=1, max_text_len=6, max_beams=2).infer(
            make_frames(1, 2, cfg.image_size, 0), beam_size=2, max_steps=4, per_node_beam_size=1, on_device=True)
    with pytest.raises(GitcapError):                                    # raw frames smaller than... zero-sized
        m._call("gitcap_greedy_raw", ptr(buf), 1, 2, 0, 0, 2, 0, ptr(buf), None, m._stream())
    assert m.weight_bytes() > 0 and m.workspace_bytes() > m.weight_bytes()


def test_pipelined_submit_matches_synchronous(captioner_cls):
    """gitcap_greedy_submit/_wait (two batches in flight on the library's streams) must give exactly
    the ids of the one-batch-at-a-time path."""
    cfg = git_tiny(2)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=4, max_text_len=8)
    batches = [make_frames(4, 2, cfg.image_size, 100 + i).cuda() for i in range(5)]
    want = [m.greedy_decode(b, max_len=8, stop="never").clone() for b in batches]
    got, pending = [], None
    for b in batches:
        fut = m.greedy_decode_async(b, max_len=8, stop="never")
        if pending is not None:
            got.append(pending.result())
        pending = fut
    got.append(pending.result())
    torch.cuda.synchronize()
    for a, b in zip(want, got):
        assert torch.equal(a, b)
    assert torch.equal(m.greedy_decode(batches[0], max_len=8, stop="never"), want[0])   # sync path still fine afterwards
    # dynamic batching: pairs of submissions run as one 8-row pass; a lone tail batch flushes on result()
    m8 = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=8, max_text_len=8)
    futs = [m8.greedy_decode_async(b, max_len=8, stop="never", coalesce=2) for b in batches]
    for a, f in zip(want, futs):
        assert torch.equal(a, f.result())
    with pytest.raises(ValueError):
        m.greedy_decode_async(batches[0], max_len=8, coalesce=2)          # 2 x 4 rows > max_batch 4


def test_pipelined_bench_shape_bitwise(captioner_cls):
    """The path the headline number is measured on (bench.py default): GIT-base, 6-frame clips, 16-clip batches, 20 tokens,
    3-4 submissions in flight on the library's streams -- the residual GEMMs' statistics exchange (gemm_epilogue.h) and the
    text block's last-arriver reducer (txtblock.hip) run while two other streams are live.  Clips are independent
    (model.py:765), so pipelining, a ragged 7-clip or single-clip batch in the rotation and coalescing two submissions into
    one 32-clip pass must not change one id: every result BITWISE equal to the synchronous greedy_decode of that input."""
    cfg = git_base(6)
    w = synthetic_weights(cfg, 0)
    m = captioner_cls(cfg, w, max_batch=16, max_frames=6, max_text_len=20, stop="never")
    g = torch.Generator().manual_seed(5)
    inputs = [torch.randn(b, 6, 3, cfg.image_size, cfg.image_size, generator=g).cuda() for b in (16, 16, 7, 16, 1)]
    want = [m.greedy_decode(x, max_len=20).clone() for x in inputs]
    torch.cuda.synchronize()
    pend, bad, n = [], [], 40
    for i in range(n):
        k = (i * 7 + i // 3) % len(inputs)
        pend.append((i, k, m.greedy_decode_async(inputs[k], max_len=20)))
        while len(pend) >= 4 - (i % 3 == 0):                   # keep 3 or 4 in flight (the library has four slots)
            j, k0, f = pend.pop(0)
            if not torch.equal(f.result(), want[k0]):
                bad.append((j, k0))
    for j, k0, f in pend:
        if not torch.equal(f.result(), want[k0]):
            bad.append((j, k0))
    assert not bad, f"pipelined submissions (index, input) differ from the synchronous call: {bad}"
    # dynamic batching at the bench shape: two 16-clip submissions as one 32-clip pass (888-tile GEMM grids), 3 passes in flight
    m32 = captioner_cls(cfg, w, max_batch=32, max_frames=6, max_text_len=20, stop="never")
    full = [k for k in range(len(inputs)) if inputs[k].shape[0] == 16]
    order = [full[i % len(full)] for i in range(12)]
    futs = [m32.greedy_decode_async(inputs[k], max_len=20, coalesce=2) for k in order]
    for k, f in zip(order, futs):
        assert torch.equal(f.result(), want[k]), ("coalesce=2", k)
    assert torch.equal(m32.greedy_decode(inputs[2], max_len=20), want[2])       # synchronous call on the same handle afterwards


def test_sync_calls_interleaved_with_submissions_in_flight(captioner_cls):
    """A synchronous call while gitcap_greedy_submit work is still running on the library's streams shares the image-row
    workspace with it: the C ABI orders the caller's stream behind every submission in flight (no device sync, no
    .result() first), and a future dropped without .result() keeps its buffers alive in the model's table."""
    cfg = git_base(2)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=4, max_frames=2, max_text_len=8)
    batches = [make_frames(4, 2, cfg.image_size, 300 + i).cuda() for i in range(4)]
    want = [m.greedy_decode(b, max_len=8, stop="never").clone() for b in batches]
    torch.cuda.synchronize()
    for rep in range(3):
        futs = [m.greedy_decode_async(b, max_len=8, stop="never") for b in batches[:3]]
        # (a) straight through the C ABI, bypassing the Python-side drain: gitcap_greedy on slot 0 right now
        ids = torch.empty((4, 9), dtype=torch.int64, device="cuda")
        steps = torch.zeros((1,), dtype=torch.int32, device="cuda")
        with torch.cuda.device(m._dev):
            m._call("gitcap_greedy", ptr(batches[3]), 4, 2, 8, 0,
                    ptr(ids), ptr(steps), m._stream())
        assert torch.equal(ids, want[3])
        # (b) the Python surface: a synchronous greedy_decode with futures outstanding, one of them never resolved
        del futs[1]
        assert torch.equal(m.greedy_decode(batches[3], max_len=8, stop="never"), want[3])
        assert torch.equal(futs[0].result(), want[0]) and torch.equal(futs[1].result(), want[2])
    # more submissions than slots without resolving any: the oldest is waited for when its slot is reused
    futs = [m.greedy_decode_async(batches[i % 4], max_len=8, stop="never") for i in range(7)]
    for i, f in enumerate(futs):
        assert torch.equal(f.result(), want[i % 4])


def test_pickle_roundtrip(captioner_cls):
    """real_time_inference.py:8-9 does torch.load() of a pickled whole module."""
    cfg = git_tiny(2)
    m = captioner_cls(cfg, synthetic_weights(cfg, 0), max_batch=2, max_text_len=8)
    fr = make_frames(2, 2, cfg.image_size, 8)
    a = m.greedy_decode(fr, max_len=6, stop="never")
    m2 = pickle.loads(pickle.dumps(m))
    m2.eval()
    assert torch.equal(m2.greedy_decode(fr, max_len=6, stop="never"), a)


def test_git_large_config_vs_oracle(captioner_cls):
    """GIT-large teacher shape (CLIPViT_L_14, visual_feature_size 1024: parameter.yaml:1-3): ViT-L/14,
    24 layers, 16 heads, 257 tokens/frame, patch 14 (patch-embed K = 588 padded to 640)."""
    from gitcap.config import git_large
    cfg = git_large(num_frames=2)
    w = synthetic_weights(cfg, 0)
    fr = make_frames(1, 2, cfg.image_size, 77)
    m = captioner_cls(cfg, w, max_batch=1, max_text_len=8)
    emul = GitOracle(cfg, w, emulate_bf16=True)
    _, vis = m.forward_image_enc(fr)
    v_e = emul.encode_frames(fr)
    assert vis.shape == (1, 2 * 257, 1024)
    assert (vis.cpu() - v_e).abs().max() < 0.06, float((vis.cpu() - v_e).abs().max())
    ids = torch.tensor([[101, 2023, 2003, 1037]])
    lg = m.forward_decoder(ids, vis).cpu()
    l_e, _ = emul.forward_output_logits(fr, ids)
    assert (lg - l_e).abs().max() < LOGIT_TOL_EMUL * 1.5, float((lg - l_e).abs().max())
    out = m.greedy_decode(fr, max_len=6, stop="never").cpu()
    _tokens_match_margin_gated(out, emul, fr)


def test_fp8_weight_values_config4(captioner_cls):
    """BASELINE configs[4] numerics: fp8 (e4m3, per-row power-of-two scale) weight values.  The oracle is
    the fp32/bf16-emulating oracle on the SAME quantised weights ('fp8 weights dequantised in the oracle',
    SURVEY.md par. 7)."""
    from gitcap.weights import is_gemm_weight, quantize_weights_fp8
    cfg = git_tiny(2)
    w = synthetic_weights(cfg, 0)
    fr = make_frames(2, 2, cfg.image_size, 31)
    m = captioner_cls(cfg, w, max_batch=2, max_text_len=8, max_beams=4, weight_dtype="fp8_e4m3")
    emul = GitOracle(cfg, quantize_weights_fp8(w), emulate_bf16=True)
    ids = torch.tensor([[101, 5, 9], [101, 77, 3]])
    lg = m(fr, ids).cpu()
    l_e, _ = emul.forward_output_logits(fr, ids)
    assert (lg - l_e).abs().max() < LOGIT_TOL_EMUL
    # e4m3 STORAGE: about half the bytes of the GEMM weights, results bitwise those of bf16 storage of the same values
    mb = captioner_cls(cfg, quantize_weights_fp8(w), max_batch=2, max_text_len=8, max_beams=4, weight_dtype="bf16")
    assert torch.equal(mb(fr, ids), m(fr, ids))
    assert torch.equal(mb.greedy_decode(fr, max_len=6, stop="never"), m.greedy_decode(fr, max_len=6, stop="never"))
    gemm_params = sum(int(np.prod(v.shape)) for k, v in w.items() if is_gemm_weight(k))
    saved = mb.weight_bytes() - m.weight_bytes()
    assert 0.8 * gemm_params < saved <= gemm_params, (saved, gemm_params)       # 2 B -> 1 B per weight (+ row scales, padding)
    bad = captioner_cls(cfg, None, max_batch=2, max_text_len=8, weight_dtype="fp8_e4m3")
    with pytest.raises(Exception, match="e4m3"):                                # unquantised values are refused, not rounded
        bad._upload(w)
    plain, _ = GitOracle(cfg, w, emulate_bf16=True).forward_output_logits(fr, ids)
    assert (lg - plain).abs().max() > 3 * (lg - l_e).abs().max()      # the quantisation is really in effect
    _tokens_match_margin_gated(m.greedy_decode(fr, max_len=6, stop="never").cpu(), emul, fr)
    assert m.infer(fr, beam_size=4, max_steps=6)["predictions"].shape == (2, 6)


def test_fp8_ffn_compute(captioner_cls):
    """compute="fp8_ffn" (north_star "MFMA bf16/fp8 GEMMs"; include/gitcap.h: gitcap_set_compute): FC1 / FC2 of the image rows on
    v_mfma_f32_16x16x128_f8f6f4 with e4m3 activations (static scale 1/16) and the e4m3 weight codes as stored.  Against the
    oracle evaluated with the same rounding points (GitOracle(emulate_fp8_act="ffn")) on a reduced 768-wide model: visual
    features and teacher-forced logits within the fp8 tolerance, the quantisation really in effect (differs from bf16 compute by
    more than it differs from its oracle), batch invariance and determinism as in bf16, and the bf16 default untouched."""
    from gitcap.config import GitCapConfig
    from gitcap.weights import quantize_weights_fp8
    cfg = GitCapConfig(image_size=64, patch_size=16, enc_width=768, enc_layers=2, enc_heads=12, enc_ffn=3072, dec_width=768,
                       dec_layers=2, dec_heads=12, dec_ffn=3072, vocab_size=997, max_text_pos=64, num_frames=3)
    wq = quantize_weights_fp8(synthetic_weights(cfg, 0))
    fr = make_frames(3, 3, cfg.image_size, 19)
    ids = torch.tensor([[101, 5, 9, 7], [101, 77, 3, 2], [101, 500, 41, 8]])
    m8 = captioner_cls(cfg, wq, max_batch=3, max_text_len=8, weight_dtype="fp8_e4m3", compute="fp8_ffn")
    mb = captioner_cls(cfg, wq, max_batch=3, max_text_len=8, weight_dtype="fp8_e4m3")
    o8 = GitOracle(cfg, wq, emulate_bf16=True, emulate_fp8_act="ffn")
    ob = GitOracle(cfg, wq, emulate_bf16=True)
    _, v8 = m8.forward_image_enc(fr)
    l8 = m8.forward_decoder(ids, v8).cpu()
    _, vb = mb.forward_image_enc(fr)
    lb = mb.forward_decoder(ids, vb).cpu()
    with torch.no_grad():
        ov8, om8 = o8.forward_image_enc(fr)
        ol8 = o8.decoder_text(o8.image_kv(om8), ids)
        ovb, omb = ob.forward_image_enc(fr)
        olb = ob.decoder_text(ob.image_kv(omb), ids)
    assert (lb - olb).abs().max() < LOGIT_TOL_EMUL * 1.5, float((lb - olb).abs().max())        # bf16 compute: unchanged
    d8 = float((l8 - ol8).abs().max())
    # an e4m3 rounding boundary moves a value by 6 % where a bf16 one moves it by 0.4 %: the device-vs-oracle noise is larger
    assert d8 < 3 * LOGIT_TOL_EMUL, d8
    assert float((v8.cpu() - ov8).abs().max()) < 0.25
    assert float((l8 - lb).abs().max()) > 0.02 and float((ol8 - olb).abs().max()) > 0.02       # the mode does something
    # batch invariance and determinism hold in fp8 compute too (same tile kernel whatever the batch)
    _, v1 = m8.forward_image_enc(fr[1:2])
    assert torch.equal(v1[0], v8[1])
    assert torch.equal(m8.greedy_decode(fr, max_len=6, stop="never")[2:], m8.greedy_decode(fr[2:], max_len=6, stop="never"))
    assert torch.equal(m8.greedy_decode(fr, max_len=6, stop="never"), m8.greedy_decode(fr, max_len=6, stop="never"))
    got = m8.greedy_decode(fr, max_len=6, stop="never").cpu()
    with torch.no_grad():                                   # teacher-force the fp8 oracle on the device's tokens (image rows through image_kv)
        tl = o8.decoder_text(o8.image_kv(om8), got[:, :-1])
    gap = tl.max(-1).values - tl.gather(2, got[:, 1:, None]).squeeze(-1)
    assert float(gap.max()) < 3 * NEAR_TIE, float(gap.max())
    with pytest.raises(ValueError, match="fp8_e4m3"):
        captioner_cls(cfg, wq, max_batch=1, max_text_len=8, compute="fp8_ffn")                 # needs e4m3 storage
    with pytest.raises(Exception, match="768 or 1024"):
        ct = git_tiny(2)
        captioner_cls(ct, quantize_weights_fp8(synthetic_weights(ct, 0)), max_batch=1, max_text_len=8, weight_dtype="fp8_e4m3", compute="fp8_ffn")


def test_more_edge_inputs(captioner_cls):
    cfg = git_tiny(2)
    w = synthetic_weights(cfg, 0)
    m = captioner_cls(cfg, w, max_batch=4, max_text_len=8)
    fr = make_frames(3, 2, cfg.image_size, 12)
    want = m.greedy_decode(fr, max_len=8, stop="never").cpu()                 # max_len == max_text_len boundary
    assert want.shape == (3, 9)
    # non-contiguous view, float64 and an odd storage offset all take the same path
    big = torch.zeros(3, 2, 3, cfg.image_size, cfg.image_size + 3, dtype=torch.float64)
    big[..., 1:cfg.image_size + 1] = fr.double()
    view = big[..., 1:cfg.image_size + 1]
    assert not view.is_contiguous()
    assert torch.equal(m.greedy_decode(view, max_len=8, stop="never").cpu(), want)
    with pytest.raises(ValueError):
        m.greedy_decode(torch.zeros(0, 2, 3, cfg.image_size, cfg.image_size), max_len=4)     # empty batch
    with pytest.raises(ValueError):
        m.greedy_decode(torch.zeros(1, 3, 3, cfg.image_size, cfg.image_size), max_len=4)     # F > max_frames
    # token ids outside the vocabulary are clamped, never read out of bounds
    _, mem = m.forward_image_enc(fr)
    y = torch.tensor([[101, 10 ** 6, -5]] * 3)
    assert torch.isfinite(m.forward_decoder(y, mem)).all()
    # two handles side by side do not share state
    m2 = captioner_cls(cfg, synthetic_weights(cfg, 1), max_batch=4, max_text_len=8)
    a2 = m2.greedy_decode(fr, max_len=8, stop="never").cpu()
    assert torch.equal(m.greedy_decode(fr, max_len=8, stop="never").cpu(), want)
    assert not torch.equal(a2, want)


def test_teacher_forward_dicts(captioner_cls):
    """GenerativeImageTextTeacher.forward (model.py:762-793): one dict per clip; 'output' = per predicted word the logits
    of the beam scoring that word highest, against the oracle's restatement of :771-788 (oracle/search_oracle.py:
    teacher_output) fed with the dict's own predictions / per-step beam logits / caption."""
    from oracle.search_oracle import teacher_output

    class SpaceTokenizer:                       # one "word" per token id, special ids dropped
        def decode(self, ids, skip_special_tokens=True):
            return " ".join(str(i) for i in ids if not (skip_special_tokens and i in (cfg.cls_token_id, cfg.sep_token_id, 0)))
    cfg = git_tiny(2)
    w = synthetic_weights(cfg, 0)
    m = captioner_cls(cfg, w, max_batch=3, max_text_len=16, max_beams=4, tokenizer=SpaceTokenizer())
    fr = make_frames(3, 2, cfg.image_size, 77)
    outs = m(fr)                                # forward(x) without y = the teacher's form (beams 4, 15 steps: model.py:702-708)
    assert isinstance(outs, list) and len(outs) == 3
    for b, r in enumerate(outs):
        assert set(r) == {"predictions", "logprobs", "logits_dict", "visual_features", "output", "cap"}
        assert r["predictions"].shape[0] == 1 and r["visual_features"].shape[0] == 1
        want = teacher_output(r["predictions"].cpu(), r["logits_dict"], r["cap"], num_beams=4)
        assert r["output"].shape == want.shape and want.shape[0] == 1 and want.shape[2] == cfg.vocab_size
        assert torch.equal(r["output"].cpu(), want)
        # the batched pass must give each clip what the reference's one-clip-at-a-time loop (model.py:765) gives it
        solo = m(fr[b:b + 1])[0]
        assert torch.equal(solo["predictions"], r["predictions"]) and torch.equal(solo["output"], r["output"])
    # without a tokenizer: cap is None, n = tokens before SEP
    m2 = captioner_cls(cfg, w, max_batch=3, max_text_len=12, max_beams=4)
    r2 = m2.teacher_forward(fr, beam_size=4, max_steps=12)
    assert r2[0]["cap"] is None and r2[0]["output"].shape[0] == 1 and r2[0]["output"].shape[2] == cfg.vocab_size


def _beam_search_matches_margin_gated(dev_out, host_out, oracle_step, oracle_search, cfg, B, beams, max_steps, length_penalty):
    """Beam search against the oracle when a device logit may differ from the oracle's by LOGIT_TOL_EMUL: the two searches
    may legitimately part where candidates tie within that noise, and not otherwise.
      1. the device-resident search == the host operator over the device's step logits (bitwise);
      2. the oracle's search loop (model.py:479-678) REPLAYED over the device's saved step logits reproduces the device's
         result exactly (the bookkeeping is the same) and yields the device's beams at every step;
      3. oracle beams vs device beams step by step: identical sets until the first step whose pruning differs; at that
         step every candidate one side kept and the other dropped lies within 2 x the measured score noise of the
         oracle's cut (and that noise is below NEAR_TIE);
      4. no divergence -> same hypothesis, logprobs within 0.05.
    Returns (and prints) one record per clip: where the two searches first part -- clip, step, measured score noise at
    that step, largest gap to the oracle's cut among the candidates kept by one side only -- or step None; and the
    device's per-step beams (for the committed device regression fixture)."""
    import torch.nn.functional as Fn
    report = []
    assert torch.equal(dev_out["predictions"], host_out["predictions"])
    assert torch.allclose(dev_out["logprobs"].cpu(), host_out["logprobs"].cpu(), atol=1e-5)
    dev_logits = [torch.as_tensor(l).float().cpu() for l in host_out["logits_dict"]]
    start = torch.full((B, 1), cfg.cls_token_id)
    dev_trace, ora_trace = [], []

    def replay(t):
        dev_trace.append(t.clone())
        return dev_logits[len(dev_trace) - 1]

    def ora(t):
        ora_trace.append(t.clone())
        return oracle_step(t)
    got = oracle_search(start, replay, eos_index=cfg.sep_token_id, max_steps=max_steps, beam_size=beams, length_penalty=length_penalty)
    assert torch.equal(got[0], dev_out["predictions"].cpu()) and torch.allclose(got[1], dev_out["logprobs"].cpu(), atol=1e-4)
    want = oracle_search(start, ora, eos_index=cfg.sep_token_id, max_steps=max_steps, beam_size=beams, length_penalty=length_penalty)
    ora_logits = want[2]
    for b in range(B):
        rows = slice(b * beams, (b + 1) * beams)
        diverged = False
        for k in range(min(len(dev_trace), len(ora_trace))):
            d, o = dev_trace[k][rows], ora_trace[k][rows]
            if sorted(map(tuple, d.tolist())) == sorted(map(tuple, o.tolist())):
                continue
            # the pruning of step k-1 differed: score every (beam, token) candidate of that step on both sides
            j = k - 1
            dj, oj = dev_trace[j][rows].tolist(), ora_trace[j][rows].tolist()
            perm = [dj.index(r) for r in oj]                      # oracle row -> device row with the same prefix
            lo = Fn.log_softmax(ora_logits[j][rows].float(), -1)
            ld = Fn.log_softmax(dev_logits[j][rows][perm], -1)
            # beam scores are sums of earlier candidates' log-probs: rebuild them per prefix from the traces
            def prefix_scores(trace, logits):
                sc = torch.zeros(beams)
                for r, pre in enumerate(trace[j][rows].tolist()):
                    tot = 0.0
                    for q in range(1, len(pre)):
                        prow = [tuple(x) for x in trace[q - 1][rows].tolist()].index(tuple(pre[:q]))
                        tot += float(Fn.log_softmax(logits[q - 1][rows][prow].float(), -1)[pre[q]])
                    sc[r] = tot
                return sc
            so = prefix_scores(ora_trace, ora_logits)
            sd = prefix_scores(dev_trace, dev_logits)[perm]
            if j == 0:
                so[1:] = -1e9; sd[1:] = -1e9                       # model.py:509: all beams start as copies of one
            co, cd = (lo + so[:, None]).flatten(), (ld + sd[:, None]).flatten()
            top = torch.unique(torch.cat([co.topk(3 * beams).indices, cd.topk(3 * beams).indices]))
            noise = float((co[top] - cd[top]).abs().max())
            assert noise < NEAR_TIE, (b, j, noise)
            V = lo.shape[-1]
            kept_o = {tuple(r) for r in o.tolist()}
            kept_d = {tuple(r) for r in d.tolist()}
            cut = min(float(co[oj.index(list(pre[:-1])) * V + pre[-1]]) for pre in kept_o)
            worst = 0.0
            for pre in kept_o ^ kept_d:
                gap = abs(float(co[oj.index(list(pre[:-1])) * V + pre[-1]]) - cut)
                assert gap <= 2 * noise + 1e-6, (b, j, pre, gap, noise)
                worst = max(worst, gap)
            report.append({"clip": b, "step": j, "noise": round(noise, 5), "gap_to_cut": round(worst, 5),
                           "dev_logprob": round(float(dev_out["logprobs"][b]), 4), "oracle_logprob": round(float(want[1][b]), 4)})
            diverged = True
            break
        if not diverged:
            assert torch.equal(dev_out["predictions"][b].cpu(), want[0][b])
            assert abs(float(dev_out["logprobs"][b].cpu() - want[1][b])) < 0.05
            report.append({"clip": b, "step": None, "dev_logprob": round(float(dev_out["logprobs"][b]), 4),
                           "oracle_logprob": round(float(want[1][b]), 4)})
    print("beam search vs oracle, first divergence per clip:", report)
    return report, dev_trace


def _check_device_regression(golden_dir, name, out, dev_trace, report):
    """The device's own result pinned against regression: ids exactly, log-probabilities to 1e-3, the
    beams of every step exactly, as the device produced them when the fixture was written (tools/gen_device_regression.py,
    run on the MI355X box).  A legitimate arithmetic change (summation order) that moves one of these is SEEN here; it is
    then judged with the margin-gated oracle comparison above and the fixture regenerated.  GITCAP_WRITE_REGRESSION=dir
    writes the fixture instead of checking it."""
    path = os.path.join(golden_dir, name)
    rec = {"predictions": out["predictions"].cpu().numpy(), "logprobs": out["logprobs"].cpu().numpy().reshape(-1),
           "n_steps": np.int64(len(dev_trace))}
    for k, t in enumerate(dev_trace):
        rec[f"beams_{k}"] = t.cpu().numpy()
    rec["first_divergence_step"] = np.array([-1 if r["step"] is None else r["step"] for r in report], np.int64)
    wdir = os.environ.get("GITCAP_WRITE_REGRESSION")
    if wdir:
        os.makedirs(wdir, exist_ok=True)
        np.savez_compressed(os.path.join(wdir, name), **rec)
        return
    if not os.path.exists(path):
        pytest.skip(f"{name} not committed yet (generate with tools/gen_device_regression.py on the GPU box)")
    g = np.load(path)
    assert np.array_equal(g["predictions"], rec["predictions"]), "device beam-search ids moved vs the committed device fixture"
    assert np.allclose(g["logprobs"], rec["logprobs"], atol=1e-3), (g["logprobs"], rec["logprobs"])
    assert int(g["n_steps"]) == len(dev_trace)
    for k in range(len(dev_trace)):
        assert np.array_equal(g[f"beams_{k}"], rec[f"beams_{k}"]), f"device beams of step {k} moved vs the committed device fixture"


def test_config4_real_shape_fp8_beam(captioner_cls, golden_dir):
    """BASELINE configs[4] at its real shape: GIT-large (ViT-L/14, parameter.yaml:1-3), 10-frame clip, e4m3 weight
    storage, beam 4, 15 steps (model.py:702-708).  Teacher-forced logits against the bf16-emulating oracle on the same
    quantised weights, and the device-resident search against the oracle's search loop (model.py:479-678) over the
    oracle's KV-free step."""
    from gitcap.config import git_large
    from gitcap.weights import quantize_weights_fp8
    from oracle.search_oracle import beam_search as oracle_beam_search
    cfg = git_large(num_frames=10)
    w = synthetic_weights(cfg, 0)
    wq = quantize_weights_fp8(w)
    del w
    fr = make_frames(1, 10, cfg.image_size, 41)
    m = captioner_cls(cfg, wq, max_batch=1, max_frames=10, max_text_len=16, max_beams=4, weight_dtype="fp8_e4m3")
    emul = GitOracle(cfg, wq, emulate_bf16=True)
    with torch.no_grad():
        _, mem = emul.forward_image_enc(fr)
        ikv = emul.image_kv(mem)                  # the image half once; every search step reruns the text rows only
    _, vis = m.forward_image_enc(fr)
    assert vis.shape == (1, 10 * 257, 1024)
    ids = torch.tensor([[101, 2023, 2003, 1037, 3899]])
    lg = m.forward_decoder(ids, vis).cpu()
    with torch.no_grad():
        l_e = emul.decoder_text(ikv, ids)
    assert (lg - l_e).abs().max() < LOGIT_TOL_EMUL * 1.5, float((lg - l_e).abs().max())
    out = m.infer(fr, beam_size=4, max_steps=15, length_penalty=0.6, on_device=True)
    host = m.infer(fr, beam_size=4, max_steps=15, length_penalty=0.6, on_device=False, save_logits=True)
    assert out["predictions"].shape == (1, 15)

    def step(t):
        with torch.no_grad():
            return emul.decoder_text(ikv, t, torch.zeros(t.shape[0], dtype=torch.long))[:, -1]
    report, dev_trace = _beam_search_matches_margin_gated(out, host, step, oracle_beam_search, cfg, 1, 4, 15, 0.6)
    _check_device_regression(golden_dir, "device_beam_cfg4.npz", out, dev_trace, report)


def test_config4_exact_fixture(captioner_cls, golden_dir):
    """BASELINE configs[4] at its real shape against a golden the device must reproduce EXACTLY:
    tests/golden/cfg4_beam_exact.npz holds the frame seed, the oracle's caption and log-probability for a clip whose
    caption is certified (oracle/gen_golden_cfg4_beam.py: a tree over every way of breaking the ties inside NEAR_TIE) not to
    depend on how a near-tie among the low beams falls; final margin to any other reachable hypothesis 0.31 (normalised).
    The same e4m3-valued GIT-large weights as test_config4_real_shape_fp8_beam; nothing from oracle/ runs here."""
    from gitcap.config import git_large
    from gitcap.weights import quantize_weights_fp8
    g = np.load(os.path.join(golden_dir, "cfg4_beam_exact.npz"))
    F, beams, steps = int(g["frames"]), int(g["beams"]), int(g["max_steps"])
    cfg = git_large(num_frames=F)
    wq = quantize_weights_fp8(synthetic_weights(cfg, int(g["weight_seed"])))
    fr = make_frames(1, F, cfg.image_size, int(g["frame_seed"]))
    want = torch.from_numpy(g["predictions"])
    for storage in ("fp8_e4m3", "bf16"):                      # e4m3 storage and bf16 storage of the same values: same bits
        m = captioner_cls(cfg, wq, max_batch=1, max_frames=F, max_text_len=16, max_beams=beams, weight_dtype=storage)
        out = m.infer(fr, beam_size=beams, max_steps=steps, length_penalty=float(g["length_penalty"]),
                      per_node_beam_size=int(g["per_node_beam_size"]), on_device=True)
        assert torch.equal(out["predictions"].cpu(), want), (storage, out["predictions"].cpu().tolist(), want.tolist())
        assert abs(float(out["logprobs"][0, 0]) - float(g["logprob"])) < 0.05, (storage, float(out["logprobs"][0, 0]), float(g["logprob"]))
        host = m.infer(fr, beam_size=beams, max_steps=steps, length_penalty=float(g["length_penalty"]),
                       per_node_beam_size=int(g["per_node_beam_size"]), on_device=False)
        assert torch.equal(host["predictions"].cpu(), want)
        del m


def test_config4_fp8_ffn_compute(captioner_cls):
    """BASELINE configs[4] at its real shape with compute="fp8_ffn" (FC1 / FC2 of the image rows on fp8 MFMA, e4m3 storage):
    teacher-forced logits against the oracle evaluated with the same e4m3 rounding points, the distance to the bf16-emulating
    oracle (what the mode costs in accuracy: the 0.3 bar of docs/LAB_NOTEBOOK.md par. 6), and the device-resident search against the host
    operator."""
    from gitcap.config import git_large
    from gitcap.weights import quantize_weights_fp8
    cfg = git_large(num_frames=10)
    wq = quantize_weights_fp8(synthetic_weights(cfg, 0))
    fr = make_frames(1, 10, cfg.image_size, 41)
    m = captioner_cls(cfg, wq, max_batch=1, max_frames=10, max_text_len=16, max_beams=4, weight_dtype="fp8_e4m3", compute="fp8_ffn")
    o8 = GitOracle(cfg, wq, emulate_bf16=True, emulate_fp8_act="ffn")
    ob = GitOracle(cfg, wq, emulate_bf16=True)
    ids = torch.tensor([[101, 2023, 2003, 1037, 3899]])
    _, vis = m.forward_image_enc(fr)
    lg = m.forward_decoder(ids, vis).cpu()
    with torch.no_grad():
        _, mem8 = o8.forward_image_enc(fr)
        ikv8 = o8.image_kv(mem8)
        l8 = o8.decoder_text(ikv8, ids)
        _, memb = ob.forward_image_enc(fr)
        lb = ob.decoder_text(ob.image_kv(memb), ids)
    d_own, d_bf16 = float((lg - l8).abs().max()), float((lg - lb).abs().max())
    print(f"configs[4] fp8_ffn: max |dlogit| device vs fp8-emulating oracle {d_own:.3f}, vs bf16-emulating oracle {d_bf16:.3f}, "
          f"fp8 oracle vs bf16 oracle {float((l8 - lb).abs().max()):.3f}")
    assert d_own < 3 * LOGIT_TOL_EMUL, d_own
    assert d_bf16 < 0.3, d_bf16                  # the accuracy bar of the mode (docs/LAB_NOTEBOOK.md par. 3): measured 0.169
    # the searches run on the same kernels: device-resident == host operator, bitwise
    out = m.infer(fr, beam_size=4, max_steps=15, length_penalty=0.6, on_device=True)
    host = m.infer(fr, beam_size=4, max_steps=15, length_penalty=0.6, on_device=False)
    assert out["predictions"].shape == (1, 15) and torch.equal(out["predictions"], host["predictions"])
    assert torch.allclose(out["logprobs"].cpu(), host["logprobs"].cpu(), atol=1e-5)


def test_device_beam_search_base_size(captioner_cls, golden_dir):
    """The device-resident beam search at GIT-base size (2 clips x 2 frames, beam 4, 10 steps) against the oracle's
    search over the oracle's step, and against the host-side operator (bitwise: same kernels make the logits)."""
    from oracle.search_oracle import beam_search as oracle_beam_search
    cfg = git_base(2)
    w = synthetic_weights(cfg, 0)
    fr = make_frames(2, 2, cfg.image_size, 52)
    m = captioner_cls(cfg, w, max_batch=2, max_frames=2, max_text_len=12, max_beams=4)
    dev = m.infer(fr, beam_size=4, max_steps=10, length_penalty=0.6, on_device=True)
    host = m.infer(fr, beam_size=4, max_steps=10, length_penalty=0.6, on_device=False, save_logits=True)
    emul = GitOracle(cfg, w, emulate_bf16=True)
    with torch.no_grad():
        _, mem = emul.forward_image_enc(fr)
        ikv = emul.image_kv(mem)

    def step(t):
        with torch.no_grad():
            return emul.decoder_text(ikv, t, torch.arange(2).repeat_interleave(4))[:, -1]
    report, dev_trace = _beam_search_matches_margin_gated(dev, host, step, oracle_beam_search, cfg, 2, 4, 10, 0.6)
    _check_device_regression(golden_dir, "device_beam_base.npz", dev, dev_trace, report)


def test_forward_output_logits_hidden_states(captioner_cls, golden_dir):
    """Third return of forward_output_logits (model.py:419-424, :747-760): per clip the decoder stack's input and the
    output of each layer over [image ; text], [dec_layers + 1, S_img + T, D]; against the bf16-emulating oracle and the
    transformers fixture (output_hidden_states=True)."""
    cfg = git_tiny(2)
    w = synthetic_weights(cfg, 0)
    g = np.load(os.path.join(golden_dir, "hf_tiny_F2.npz"))
    fr = make_frames(2, 2, cfg.image_size, int(g["frame_seed"]))
    ids = torch.from_numpy(g["prefix_ids"])
    m = captioner_cls(cfg, w, max_batch=2, max_text_len=8)
    logits, vis, hid = m.forward_output_logits(fr, ids, output_hidden_states=True)
    assert len(hid) == 2 and tuple(hid[0].shape) == (cfg.dec_layers + 1, 2 * cfg.tokens_per_frame + ids.shape[1], cfg.dec_width)
    got = torch.stack([h.cpu() for h in hid], 1)                          # [L+1, B, S, D] like the fixture
    emul = GitOracle(cfg, w, emulate_bf16=True)
    _, mem = emul.forward_image_enc(fr)
    _, want = emul.decoder_full(mem, ids, return_hidden=True)
    assert (got - torch.stack(want, 0)).abs().max() < 0.06, float((got - torch.stack(want, 0)).abs().max())
    assert np.abs(got.numpy() - g["hidden"]).max() < 0.12                 # fp32 transformers fixture (hidden std ~1)
    # the default call is unchanged (no hidden states, same logits), also right after an exporting call
    l2, _, h2 = m.forward_output_logits(fr, ids)
    assert h2 == [] and torch.equal(torch.cat(l2), torch.cat(logits))
    assert torch.equal(m.greedy_decode(fr, max_len=6, stop="never"), captioner_cls(cfg, w, max_batch=2, max_text_len=8).greedy_decode(fr, max_len=6, stop="never"))
