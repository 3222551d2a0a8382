"""What the GPU tests share: the `lib` / `captioner_cls` fixtures, tensors as C-ABI arguments, poisoned output buffers and their
tail checks, the derived-bound comparison with an fp64 reference, the runner of the vocabulary-head debug hooks, the beam
buffers of the gitcap_dbg_beam_* hooks and the small models several modules build.

New GPU tests import from here (tests/ is on sys.path, as for the *_reference.py modules); a fixture is taken with
`from gpu_support import lib  # noqa: F401`, since pytest collects the fixtures it finds in a test module's namespace.
Importing this module needs neither a GPU nor the built library."""
import collections
import ctypes
import math

import numpy as np
import pytest
import torch

from text_rows_reference import flip_share

NAN = float("nan")
NINF = float("-inf")


# ---- fixtures -----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    from gitcap import _lib
    assert torch.cuda.is_available()
    return _lib.load()


@pytest.fixture(scope="module")
def captioner_cls():
    from gitcap.model import GitCaptioner
    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    return GitCaptioner


# ---- tensors as arguments, results as arrays ------------------------------------------------------------------------------------

def ptr(t):
    """tensor -> c_void_p of its data; None -> None (NULL for an argument declared c_void_p)"""
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def to_dev(a, dtype):
    """array (or nested list) -> device tensor of `dtype`; None -> None"""
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).to(device="cuda", dtype=dtype)


def f64(t):
    return t.detach().float().cpu().numpy().astype(np.float64)


def bf16_bits(t):
    return t.contiguous().view(torch.int16).cpu().numpy().view(np.uint16)


def same_bits(a, b):
    """bitwise equal, NaN poison included"""
    return torch.equal(a.view(torch.int16) if a.dtype == torch.bfloat16 else a.view(torch.int32),
                       b.view(torch.int16) if b.dtype == torch.bfloat16 else b.view(torch.int32))


def rms(t):
    return float(t.double().pow(2).mean().sqrt())


def camera(shape, seed):
    """uint8 camera frames on the host, e.g. shape [B, F, H, W, 3]"""
    return torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(seed))


# ---- the derived-bound check ----------------------------------------------------------------------------------------------------

def close_to_fp64(dev, ref, bound, what, flips=True):
    """max |device - fp64| / bound <= 1, and (flips) at most 2 % of the elements off the correctly rounded reference"""
    dev, ref = np.asarray(dev, np.float64), np.asarray(ref, np.float64)
    assert not np.isnan(dev).any(), what
    ratio = float((np.abs(dev - ref) / bound).max())
    share = flip_share(dev, ref) if flips else 0.0
    print(f"{what}: max |device - fp64| / bound = {ratio:.3f}" + (f", share off the correctly rounded value {share:.4f}" if flips else ""))
    assert ratio <= 1.0, what
    assert share <= 0.02, what


# ---- poisoned buffers -----------------------------------------------------------------------------------------------------------

def poisoned(count, fill, dtype=torch.float32):
    """A device buffer of `count` elements (or of a shape) that holds `fill` everywhere: larger than the kernel may write."""
    return torch.full((count,) if isinstance(count, int) else tuple(count), fill, device="cuda", dtype=dtype)


def assert_tail(buf, used, fill):
    """Nothing behind the first `used` elements of a poisoned buffer was written."""
    tail = buf.reshape(-1)[used:]
    assert bool(torch.isnan(tail).all()) if isinstance(fill, float) and math.isnan(fill) else bool((tail == fill).all())


# ---- the vocabulary head's debug hooks --------------------------------------------------------------------------------------------

IDX_FILL = -5                   # pre-fill of the arg-max indices
TGT_FILL = -777.25              # pre-fill of tgt_logit

HeadOut = collections.namedtuple("HeadOut", "logits val idx sum tgt_logit")


def e4m3_rows(Wf):
    """fp32 rows -> (e4m3 codes, the power-of-two row scale 2^ceil(log2(amax / 448)), the values the codes stand for)"""
    wscale = torch.exp2(torch.ceil(torch.log2(Wf.abs().amax(dim=1) / 448.0)))
    W = (Wf / wscale[:, None]).to(torch.float8_e4m3fn)
    return W, wscale, W.float() * wscale[:, None]


def softmax_head_inputs(M, N, K, fp8, seed, ninf=False):
    """Head operands whose logits have the shape of a softmax (tests/test_logprob_gpu.py, tests/test_score_gpu.py) -> X, W, wscale, bias"""
    g = torch.Generator(device="cuda").manual_seed(seed)
    Np = (N + 15) // 16 * 16
    X = torch.randn(M, K, device="cuda", generator=g).bfloat16()
    Wf = torch.randn(Np, K, device="cuda", generator=g) * (3.0 / K ** 0.5)        # logits of a few units: a softmax with a shape
    bias = torch.randn(N, device="cuda", generator=g)
    for n in range(N, Np):                          # padding rows: a missing n < N guard would put e^large into the last tile's sum
        Wf[n] = 4.0 * X[n % M].float()
    if ninf:
        if N >= 32:
            bias[16:32] = NINF                      # a whole tile: the 0-sum rule
        bias[torch.arange(1, N, 7, device="cuda")] = NINF
    if fp8:
        W, wscale, _ = e4m3_rows(Wf)
    else:
        wscale, W = None, Wf.bfloat16()
    return X, W, wscale, bias


def run_vocab_head(lib, X, ldx, W, wscale, bias, M, N, K, *, share=1, hook="plain", targets=None, want_logits=True):
    """One launch of gitcap_dbg_vocab_head ("plain"), _lse or _score under head form `share` (gitcap_dbg_config(10, .)) ->
    HeadOut(logits [M][N], val, idx, sum [M][nt], tgt_logit [M]), None for what the hook does not produce.  Every buffer is 16
    elements longer than the launch may write; the tails (and, under "plain", the whole sum buffer) are checked."""
    assert hook in ("plain", "lse", "score") and (hook == "score") == (targets is not None)
    nt = (N + 15) // 16
    logits = poisoned(M * N + 16, NAN) if want_logits else None
    val = poisoned(M * nt + 16, NAN)
    idx = poisoned(M * nt + 16, IDX_FILL, torch.int32)
    ssum = poisoned(M * nt + 16, NAN)
    tl = poisoned(M + 16, TGT_FILL) if hook == "score" else None
    tg = to_dev(targets, torch.int64)
    head = (ptr(X), ldx, ptr(W), ptr(wscale), ptr(bias), M, N, K, ptr(logits), ptr(val), ptr(idx))
    old = lib.gitcap_dbg_config(10, share)
    try:
        if hook == "plain":
            rc = lib.gitcap_dbg_vocab_head(*head, stream())
        elif hook == "lse":
            rc = lib.gitcap_dbg_vocab_head_lse(*head, ptr(ssum), stream())
        else:
            rc = lib.gitcap_dbg_vocab_head_score(*head, ptr(ssum), ptr(tg), ptr(tl), stream())
        torch.cuda.synchronize()
    finally:
        lib.gitcap_dbg_config(10, old)
    assert rc == 0
    if want_logits:
        assert_tail(logits, M * N, NAN)
    assert_tail(val, M * nt, NAN)
    assert_tail(idx, M * nt, IDX_FILL)
    assert_tail(ssum, 0 if hook == "plain" else M * nt, NAN)
    if hook == "score":
        assert_tail(tl, M, TGT_FILL)
    return HeadOut(logits[:M * N].view(M, N) if want_logits else None, val[:M * nt].view(M, nt), idx[:M * nt].view(M, nt),
                   ssum[:M * nt].view(M, nt) if hook != "plain" else None, tl[:M] if hook == "score" else None)


# ---- beam buffers ---------------------------------------------------------------------------------------------------------------

def beam_state(B, beams, n, L):
    """The buffers of the gitcap_dbg_beam_* hooks, poisoned -> (dict of tensors, CDbgBeamBuffers, CDbgBeamBuffersNbest)"""
    from gitcap._lib import CDbgBeamBuffers, CDbgBeamBuffersNbest
    rows = B * beams
    i64, i32 = torch.int64, torch.int32
    t = dict(ids0=poisoned((rows, L), -777, i64), ids1=poisoned((rows, L), -777, i64), words=poisoned(rows, -777, i64),
             hyp_ids=poisoned((B, n, L), -777, i64), beam_scores=poisoned(rows, NAN), hyp_score=poisoned((B, n), NAN),
             src_rows=poisoned(rows, -777, i32), done=poisoned(B, -777, i32), hyp_len=poisoned((B, n), -777, i32))
    order = ("ids0", "ids1", "words", "hyp_ids", "beam_scores", "hyp_score", "src_rows", "done", "hyp_len")
    ptrs = [t[k].data_ptr() for k in order]
    return t, CDbgBeamBuffers(*ptrs), CDbgBeamBuffersNbest(*ptrs, n)


# ---- models ---------------------------------------------------------------------------------------------------------------------

def student_cfg(name):
    from gitcap.student_config import student_base, student_tiny
    return student_tiny() if name == "tiny" else student_base()


def tinyvit_cfg(name, *mem_shape):
    from gitcap.tinyvit_config import tinyvit_config, tinyvit_tiny
    return tinyvit_tiny(*mem_shape) if name == "tiny" else tinyvit_config("tiny_vit_21m_224", *mem_shape)


def make_student(name, seed=0, **kw):
    from gitcap.student import StudentCaptioner
    from gitcap.student_config import student_synthetic_weights
    cfg = student_cfg(name)
    return StudentCaptioner(cfg=cfg, weights=student_synthetic_weights(cfg, seed), device="cuda:0", **kw)


def make_student_native(name, *, tinyvit=None, **kw):
    """The student with the native TinyViT encoder of size `tinyvit` (default: the student's own name), both with seed 0."""
    from gitcap.student import StudentCaptioner
    from gitcap.student_config import student_synthetic_weights
    from gitcap.tinyvit import TinyViTEncoder
    from gitcap.tinyvit_config import tinyvit_synthetic_weights
    tcfg, scfg = tinyvit_cfg(tinyvit or name), student_cfg(name)
    weights = dict(student_synthetic_weights(scfg, 0))
    weights.update({"image_encoder.model." + k: v for k, v in tinyvit_synthetic_weights(tcfg, 0).items()})
    enc = TinyViTEncoder(tcfg, device="cuda:0", max_frames=kw.get("max_batch", 4) * scfg.mem_tokens)
    return StudentCaptioner(cfg=scfg, weights=weights, image_encoder=enc, device="cuda:0", **kw)


def make_encoder(name, max_frames=8):
    from gitcap.tinyvit import TinyViTEncoder
    from gitcap.tinyvit_config import tinyvit_synthetic_weights
    cfg = tinyvit_cfg(name)
    return TinyViTEncoder(cfg, tinyvit_synthetic_weights(cfg, 0), device="cuda:0", max_frames=max_frames)


def mid768(dec_layers=2):
    """The 768-wide mid-size GIT: two encoder blocks, a vocabulary of 997, three frames of 64 x 64."""
    from gitcap.config import GitCapConfig
    return GitCapConfig(image_size=64, patch_size=16, enc_width=768, enc_layers=2, enc_heads=12, enc_ffn=3072, dec_width=768,
                        dec_layers=dec_layers, dec_heads=12, dec_ffn=3072, vocab_size=997, max_text_pos=64, num_frames=3)
