"""The three wrappers over gitcap._handle._NativeModule on the device (tiny configs): to() that moves nothing, the refused
to("cpu"), the family's own last-error text behind a refused call, and a real move of the student with its native encoder."""
import re

import pytest
import torch

from gitcap import _lib
from gitcap.config import git_tiny
from gitcap.student_config import student_synthetic_weights, student_tiny
from gitcap.tinyvit_config import tinyvit_synthetic_weights, tinyvit_tiny
from gitcap.weights import synthetic_weights

pytestmark = pytest.mark.gpu
MAX_LEN = 8


def _frames(shape, seed):
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to("cuda:0")


def _student_weights():
    w = dict(student_synthetic_weights(student_tiny(), 0))
    w.update({"image_encoder.model." + k: v for k, v in tinyvit_synthetic_weights(tinyvit_tiny(), 0).items()})
    return w


def _git():
    from gitcap.model import GitCaptioner
    cfg = git_tiny(2)
    m = GitCaptioner(cfg, synthetic_weights(cfg, 0), device="cuda:0", max_batch=2, max_text_len=MAX_LEN)
    fr = _frames((2, 2, 3, cfg.image_size, cfg.image_size), 1)
    ids, steps = torch.empty((1, MAX_LEN + 2), dtype=torch.int64, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0")
    refused = lambda: m._call("gitcap_greedy", _lib.ptr(fr), 1, 2, MAX_LEN + 1, 0, _lib.ptr(ids), _lib.ptr(steps), m._stream())
    return m, (lambda: m.greedy_decode(fr, max_len=MAX_LEN, stop="never")), ("gitcap_greedy", refused)


def _student(device="cuda:0"):
    from gitcap.student import StudentCaptioner
    from gitcap.tinyvit import TinyViTEncoder
    scfg, tcfg = student_tiny(), tinyvit_tiny()
    enc = TinyViTEncoder(tcfg, device=device, max_frames=2 * scfg.mem_tokens)
    m = StudentCaptioner(cfg=scfg, weights=_student_weights(), image_encoder=enc, device=device, max_batch=2, max_text_len=MAX_LEN)
    fr = _frames((2, scfg.mem_tokens, 3, tcfg.img_size, tcfg.img_size), 2)
    mem = torch.zeros((1, scfg.mem_tokens, scfg.d_model), device="cuda:0")
    ids, steps = torch.empty((1, MAX_LEN + 2), dtype=torch.int64, device="cuda:0"), torch.zeros(1, dtype=torch.int32, device="cuda:0")
    refused = lambda: m._call("gitcap_student_greedy", _lib.ptr(mem), 1, MAX_LEN + 1, 0, _lib.ptr(ids), _lib.ptr(steps), m._stream())
    return m, (lambda: m.greedy_decode(fr, max_len=MAX_LEN, stop="never")), ("gitcap_student_greedy", refused)


def _tinyvit():
    from gitcap.tinyvit import TinyViTEncoder
    cfg = tinyvit_tiny()
    m = TinyViTEncoder(cfg, tinyvit_synthetic_weights(cfg, 0), device="cuda:0", max_frames=4)
    fr = _frames((1, 2, 3, cfg.img_size, cfg.img_size), 3)
    x, mem = fr[0].contiguous(), torch.empty((2, m.out_dim), device="cuda:0")
    refused = lambda: m._call("gitcap_tinyvit_encode", _lib.ptr(x), 0, _lib.ptr(mem), None, m._stream())      # 0 frames
    return m, (lambda: m.memory(fr)), ("gitcap_tinyvit_encode", refused)


@pytest.fixture(scope="module", params=["git", "student", "tinyvit"])
def wrapper(request):
    """(module, run() -> ids / tokens of fixed inputs, (symbol, a call of it that the library's argument checks refuse))."""
    return {"git": _git, "student": _student, "tinyvit": _tinyvit}[request.param]()


def test_to_the_device_it_is_on_keeps_the_handle_and_the_bits(wrapper):
    m, run, _ = wrapper
    before, h, value = run().clone(), m._handle, m._handle.value
    for dev in ("cuda:0", torch.device("cuda", 0)):
        assert m.to(dev) is m
    assert m._handle is h and m._handle.value == value and m._dev == torch.device("cuda", 0)
    assert torch.equal(run(), before)


def test_to_cpu_is_refused_and_the_model_goes_on(wrapper):
    m, run, _ = wrapper
    before, value = run().clone(), m._handle.value
    with pytest.raises(_lib.GitcapError) as e:
        m.to("cpu")
    assert str(e.value) == "gitcap has no CPU path; .to(cpu) refused"
    assert m._handle.value == value and torch.equal(run(), before)


def test_a_refused_call_carries_its_family_s_error_text(wrapper):
    m, run, (symbol, refused) = wrapper
    before = run().clone()
    with pytest.raises(_lib.GitcapError) as e:
        refused()
    got = re.fullmatch(re.escape(symbol) + r" failed \(status (-?\d+)\): (.+)", str(e.value))
    assert got and int(got.group(1)) != 0 and got.group(2) != "?", str(e.value)      # '?' = a last_error that knew nothing of it
    assert not isinstance(e.value, _lib.GitcapExchangeTimeout)
    assert torch.equal(run(), before)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two devices")
def test_the_student_moves_with_its_encoder():
    m, run, _ = _student()
    before = run().cpu()
    st = m.caption_stream(batch=1, max_len=MAX_LEN)
    assert m.to("cuda:1") is m
    assert m._dev.index == 1 and m.image_encoder.device.index == 1
    assert torch.equal(run().cpu(), before)
    with pytest.raises(_lib.GitcapError, match="StudentCaptionStream was invalidated"):
        st.reset()
