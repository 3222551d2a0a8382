"""Live captioning on the student, the parts that need no device: the five entry points (gitcap_tinyvit_encode_raw,
gitcap_student_window_reset / _push / _greedy / _beam_search) are bound and exported, refuse a null handle before touching a
device, their kernels are in the gfx950 code object and compile without scratch.  The device tests are in
test_student_live_gpu.py."""
import ctypes
import os
import sys

import pytest

from gitcap import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

NEW_SYMBOLS = ("gitcap_tinyvit_encode_raw", "gitcap_student_window_reset", "gitcap_student_window_push",
               "gitcap_student_window_greedy", "gitcap_student_window_beam_search")
NEW_KERNELS = (("preproc.hip", "preprocess_stem_kernel"), ("student.hip", "student_window_stage_kernel"),
               ("student.hip", "student_window_gather_kernel"))
EXPECTED_HIPCC = "7.2"          # the compiler tests/test_isa_lint.py takes its expectations from; same skip / xfail rule


def test_symbols_are_bound_and_exported():
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in _lib.SYMBOLS, name
        assert hasattr(lib, name), name


def test_kernels_are_in_the_gfx950_code_object():
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"gfx950" in blob
    for _, kernel in NEW_KERNELS:
        assert kernel.encode() in blob, kernel


def test_null_handle_is_refused_without_a_device():
    lib = _lib.load()
    buf = (ctypes.c_char * 64)()           # a non-null host pointer: must never be dereferenced
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert lib.gitcap_student_window_reset(None, 1) == -1
    assert lib.gitcap_student_last_error(None)
    assert lib.gitcap_student_window_push(None, p, 1, 1, None) == -1
    assert lib.gitcap_student_window_greedy(None, 4, 0, p, p, None) == -1
    assert lib.gitcap_student_window_beam_search(None, 2, 4, p, None) == -1
    assert b"null handle" in lib.gitcap_student_last_error(None)
    assert lib.gitcap_tinyvit_encode_raw(None, p, 1, 4, 4, p, None, None) == -1
    assert b"null handle" in lib.gitcap_tinyvit_last_error(None)


def _hipcc_state():
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        return "missing", "needs /opt/rocm/bin/hipcc"
    from isa_waits import hipcc_version
    v = hipcc_version()
    if v == EXPECTED_HIPCC:
        return "ok", ""
    return "other", f"ISA expectations were taken with hipcc {EXPECTED_HIPCC}, this is {v}"


_state, _why = _hipcc_state()
_lint_mark = (pytest.mark.skip(reason=_why) if _state == "missing"
              else pytest.mark.xfail(reason=_why, strict=False) if _state == "other" else lambda f: f)


@_lint_mark
def test_new_kernels_use_no_scratch():
    from isa_waits import kernel_listings
    for src, kernel in NEW_KERNELS:
        res, _ = kernel_listings(src, kernel)
        assert len(res) == 1, (src, kernel, [r[0] for r in res])
        name, vgprs, scratch, toks = res[0]
        print(f"{src}: {name}: {vgprs} VGPRs, {scratch} B scratch")
        assert scratch == 0, f"{src}: {name} uses {scratch} bytes of scratch"
        assert "xs" not in toks and "xl" not in toks, f"{src}: {name} has scratch traffic"


@_lint_mark
def test_tinyvit_kernels_use_no_scratch():
    """tinyvit.hip is not in test_isa_lint.py's file list; the raw entry point lives there, so its kernels are linted here."""
    from isa_waits import kernel_listings
    res, _ = kernel_listings("tinyvit.hip", "_Z")
    assert len(res) >= 10
    for name, vgprs, scratch, toks in res:
        assert scratch == 0, f"tinyvit.hip: {name} uses {scratch} bytes of scratch"


def test_stream_refuses_a_model_without_native_encoder():
    """caption_stream's precondition is checked in Python before any library call."""
    from gitcap.student import StudentCaptioner

    class _Fake:
        _native = lambda self: False
    with pytest.raises(_lib.GitcapError, match="native"):
        StudentCaptioner.caption_stream(_Fake())
