"""gitcap._handle._NativeModule, gitcap._stream._WindowStream and gitcap._lib.ptr without a device: the handle's life cycle, to(),
the status -> exception mapping and the greedy truncation, against a fake library that records its calls."""
import ctypes

import numpy as np
import pytest
import torch

from gitcap import _lib
from gitcap._handle import _NativeModule
from gitcap._stream import STOP_ALL_SEP, STOP_NEVER, _WindowStream
from gitcap.window import WindowSchedule

ORDER = ("b", "a", "c")                  # the subclass's own upload order (not the dict's, not sorted)


class _FakeLib:
    """x_create / x_destroy / x_last_error / x_load_tensor / x_finalize / x_op: every call is appended to `log`."""

    def __init__(self):
        self.log, self.create_rc, self.op_rc, self.msg, self.made = [], 0, 0, b"boom", 0

    def x_create(self, cfg, idx, out):
        self.log.append(("create", idx))
        if self.create_rc == 0:
            self.made += 1
            out._obj.value = 0x1000 * self.made          # `out` is ctypes.byref(handle)
        return self.create_rc

    def x_destroy(self, h):
        self.log.append(("destroy", h.value))

    def x_last_error(self, h):
        self.log.append(("last_error", None if h is None else h.value))
        return self.msg

    def x_load_tensor(self, h, name, data, shape, ndim):
        self.log.append(("load", name.decode(), tuple(shape[:ndim])))
        return 0

    def x_finalize(self, h):
        self.log.append(("finalize",))
        return 0

    def x_op(self, h, *args):
        self.log.append(("op",) + args)
        return self.op_rc

    gitcap_last_error = x_last_error                     # what GitCaptioner's family consults


class _X(_NativeModule):
    _PREFIX, _FINALIZE = "x", "x_finalize"

    def __init__(self, lib, index=0, weights=None):
        super().__init__()
        self._lib, self._dev, self._handle, self._weights = lib, torch.device("cuda", index), None, weights
        self._open()

    def _open(self):                                     # the base's _open minus its two questions to the device
        self._create_on(self._dev.index)

    def _cconfig(self):
        return ctypes.c_int(7)

    def _configure(self):
        self._lib.log.append(("configure", self._handle.value))

    def _upload(self, w):                                # the base's _load_tensors minus its torch.cuda.device block
        for name in ORDER:
            arr = np.ascontiguousarray(w[name], dtype=np.float32)
            self._call("x_load_tensor", name.encode(), arr.ctypes.data_as(ctypes.c_void_p), (ctypes.c_int64 * arr.ndim)(*arr.shape), arr.ndim)
        self._call(self._FINALIZE)

    def _moved(self):
        self._lib.log.append(("moved", self._dev.index))


def _weights():
    return {"a": np.zeros((2, 3), np.float32), "b": np.zeros((4,), np.float32), "c": np.zeros((1, 1, 5), np.float32)}


def test_close_is_idempotent_and_del_after_it_is_silent():
    lib = _FakeLib()
    m = _X(lib)
    assert lib.log == [("create", 0), ("configure", 0x1000)]
    m._close()
    m._close()
    assert m._handle is None and lib.log.count(("destroy", 0x1000)) == 1
    m.__del__()
    assert [c for c in lib.log if c[0] == "destroy"] == [("destroy", 0x1000)]
    live = _X(lib)
    live.__del__()                                       # a live object's __del__ does destroy, once
    live.__del__()
    assert [c for c in lib.log if c[0] == "destroy"] == [("destroy", 0x1000), ("destroy", 0x2000)]
    _X.__new__(_X).__del__()                             # __init__ never ran: no _handle, no _lib, no exception


def test_to_the_same_index_calls_nothing():
    lib = _FakeLib()
    m = _X(lib, index=2, weights=_weights())
    h = m._handle
    del lib.log[:]
    assert m.to("cuda:2") is m and m.to(device=torch.device("cuda", 2)) is m and m.to(torch.float16) is m
    assert lib.log == [] and m._handle is h and m._dev == torch.device("cuda", 2)


def test_to_another_index_reopens_uploads_and_reports_in_order():
    lib = _FakeLib()
    m = _X(lib, index=0, weights=_weights())
    del lib.log[:]
    assert m.to("cuda:3") is m
    assert lib.log == [("destroy", 0x1000), ("create", 3), ("configure", 0x2000), ("load", "b", (4,)), ("load", "a", (2, 3)),
                       ("load", "c", (1, 1, 5)), ("finalize",), ("moved", 3)]
    assert m._dev == torch.device("cuda", 3) and m._handle.value == 0x2000
    bare = _X(lib, index=0)                              # no weights stored: nothing to upload, _moved still runs
    del lib.log[:]
    bare.to("cuda:1")
    assert [c[0] for c in lib.log] == ["destroy", "create", "configure", "moved"]


def test_failed_recreate_in_to_leaves_nothing_to_free_twice():
    lib = _FakeLib()
    m = _X(lib, index=0, weights=_weights())
    del lib.log[:]
    lib.create_rc = -3
    with pytest.raises(_lib.GitcapError, match=r"x_create failed \(status -3\): boom"):
        m.to("cuda:1")
    assert m._handle is None
    assert lib.log == [("destroy", 0x1000), ("create", 1), ("last_error", None)]      # a failed create has no handle to ask
    m.__del__()
    assert [c for c in lib.log if c[0] == "destroy"] == [("destroy", 0x1000)]


def test_to_cpu_is_refused_before_any_call():
    lib = _FakeLib()
    m = _X(lib)
    h = m._handle
    del lib.log[:]
    for dev in ("cpu", torch.device("cpu")):
        with pytest.raises(_lib.GitcapError) as e:
            m.to(dev)
        assert str(e.value) == "gitcap has no CPU path; .to(cpu) refused"
    with pytest.raises(_lib.GitcapError, match=r"no CPU path; \.to\(cpu\) refused"):
        m.to(device="cpu")
    assert lib.log == [] and m._handle is h


def test_open_refuses_a_cpu_device_and_a_machine_without_one():
    class _Plain(_X):
        _open = _NativeModule._open
    lib = _FakeLib()
    m = _Plain.__new__(_Plain)
    torch.nn.Module.__init__(m)
    m._lib, m._dev, m._handle = lib, torch.device("cpu"), None
    with pytest.raises(_lib.GitcapError) as e:
        m._open()
    assert str(e.value) == "gitcap runs on an AMD GPU only (no CPU path); got device cpu"
    if not torch.cuda.is_available():                    # (with a device the same call goes on to x_create)
        with pytest.raises(_lib.GitcapError) as e:
            _Plain(lib)
        assert str(e.value) == "no HIP device visible: gitcap has no CPU fallback"
    assert lib.log == []


def test_call_maps_a_status_through_the_family_s_last_error():
    lib = _FakeLib()
    m = _X(lib)
    del lib.log[:]
    m._call("x_op", 1, 2)
    assert lib.log == [("op", 1, 2)]
    lib.op_rc = -2
    with pytest.raises(_lib.GitcapError) as e:
        m._call("x_op")
    assert str(e.value) == "x_op failed (status -2): boom" and type(e.value) is _lib.GitcapError
    assert lib.log[-1] == ("last_error", 0x1000)         # asked of x_last_error, with the handle
    lib.msg = None
    with pytest.raises(_lib.GitcapError) as e:
        m._call("x_op")
    assert str(e.value) == "x_op failed (status -2): ?"


def test_exchange_status_through_gitcaptioner_s_call():
    """GitCaptioner._call on GITCAP_ERR_EXCHANGE (-5): what is in flight is poisoned first, then GitcapExchangeTimeout is raised
    with the message of gitcap_last_error.  (No handle is opened: __new__ and the attributes _call reads.)"""
    from gitcap.model import GitCaptioner

    class _Sub:
        poisoned = False

    lib = _FakeLib()
    lib.op_rc = _lib.ERR_EXCHANGE
    m = GitCaptioner.__new__(GitCaptioner)
    torch.nn.Module.__init__(m)
    m._lib, m._handle, m._inflight, m._undelivered = lib, ctypes.c_void_p(0x77), [_Sub()], {_Sub()}
    with pytest.raises(_lib.GitcapExchangeTimeout) as e:
        m._call("x_op")
    assert str(e.value) == "x_op failed (status -5): boom" and lib.log[-1] == ("last_error", 0x77)
    assert all(s.poisoned for s in m._inflight) and all(s.poisoned for s in m._undelivered)
    m._handle = None                                     # nothing to destroy when `m` goes
    x = _X(lib)                                          # the same status from another family is a GitcapExchangeTimeout too:
    with pytest.raises(_lib.GitcapExchangeTimeout):      # _lib.check is the only place that maps it
        x._call("x_op")


def test_ptr():
    assert _lib.ptr(None).value is None
    t = torch.arange(6, dtype=torch.float32)
    p = _lib.ptr(t)
    assert isinstance(p, ctypes.c_void_p) and p.value == t.data_ptr()
    assert _lib.ptr(t[2:]).value == t.data_ptr() + 8


# ---------------------------------------------------------------------------------------------------- _WindowStream
class _Model:
    _dev = torch.device("cpu")
    _window_owner = None


class _Stream(_WindowStream):
    def __init__(self, model, mode=STOP_ALL_SEP, logprobs=True, max_len=6):
        self.calls = []
        super().__init__(model, WindowSchedule(2, 3, 1), max_len, mode, None, logprobs)

    def _reset_lib(self):
        self.calls.append("reset_lib")

    def _clear(self):
        self.calls.append("clear")


class OtherStream(_Stream):
    pass


def _buffers(st, steps):
    ids, st_buf, lp = st._greedy_buffers(2)
    assert ids.shape == (2, 7) and ids.dtype == torch.int64 and st_buf.shape == (1,) and st_buf.dtype == torch.int32
    ids.copy_(torch.arange(14).view(2, 7))
    st_buf.fill_(steps)
    if lp is not None:
        assert lp.shape == (2, 6) and lp.dtype == torch.float32
        lp.copy_(torch.arange(12, dtype=torch.float32).view(2, 6))
    return ids, st_buf, lp


def test_finish_greedy_truncates_only_under_all_sep_and_slices_the_logprobs():
    st = _Stream(_Model(), STOP_ALL_SEP)
    assert st.calls == ["reset_lib"]                     # opening a stream empties the library's window
    ids, steps, lp = _buffers(st, 4)
    out = st._finish_greedy(ids, steps, lp, False)
    assert torch.equal(out, ids[:, :5]) and torch.equal(st.last_logprobs, lp[:, :4])
    st = _Stream(_Model(), STOP_NEVER)
    ids, steps, lp = _buffers(st, 4)
    out = st._finish_greedy(ids, steps, lp, False)
    assert torch.equal(out, ids) and torch.equal(st.last_logprobs, lp)          # 1 + max_len ids, max_len log-probs
    st = _Stream(_Model(), STOP_ALL_SEP, logprobs=False)
    ids, steps, lp = _buffers(st, 0)
    assert lp is None
    assert st._finish_greedy(ids, steps, lp, False).shape == (2, 1) and st.last_logprobs is None


class _DeviceTensor:
    """Stands for a device tensor [rows, cols] where there is no device: column slices and .cpu(), which says where it went."""

    def __init__(self, shape, where="device"):
        self.shape, self.where = tuple(shape), where

    def __getitem__(self, idx):
        return _DeviceTensor((self.shape[0], len(range(self.shape[1])[idx[1]])), self.where)

    def cpu(self):
        return _DeviceTensor(self.shape, "cpu")


def test_finish_greedy_returns_cpu_tensors_iff_asked():
    st = _Stream(_Model(), STOP_NEVER)
    ids, lp = _DeviceTensor((2, 7)), _DeviceTensor((2, 6))
    out = st._finish_greedy(ids, None, lp, False)
    assert (out.where, out.shape, st.last_logprobs.where, st.last_logprobs.shape) == ("device", (2, 7), "device", (2, 6))
    out = st._finish_greedy(ids, None, lp, True)
    assert (out.where, out.shape, st.last_logprobs.where, st.last_logprobs.shape) == ("cpu", (2, 7), "cpu", (2, 6))
    st = _Stream(_Model(), STOP_ALL_SEP)                 # on real (CPU) tensors .cpu() keeps the values
    ids, steps, lp = _buffers(st, 2)
    out = st._finish_greedy(ids, steps, lp, True)
    assert out.device.type == "cpu" and torch.equal(out, ids[:, :3]) and torch.equal(st.last_logprobs, lp[:, :2])


def test_a_superseded_stream_refuses_reset_and_push_by_its_own_name():
    m = _Model()
    old = _Stream(m)
    new = OtherStream(m)
    del old.calls[:], new.calls[:]
    for call in (old.reset, lambda: old.push(torch.zeros((2, 1, 4)))):
        with pytest.raises(_lib.GitcapError) as e:
            call()
        assert str(e.value) == "this _Stream was invalidated (another caption_stream() was opened, or the model was moved)"
    assert old.calls == [] and old._sched.pushed == 0
    new._sched.push(2, 2)
    new.reset()
    assert new.calls == ["reset_lib", "clear"] and new._sched.pushed == 0
    m._window_owner = None                               # what a moved model does
    with pytest.raises(_lib.GitcapError, match="this OtherStream was invalidated"):
        new.reset()
    assert new.calls == ["reset_lib", "clear"]


def test_the_stop_constants_are_one_pair():
    import gitcap._stream as s
    import gitcap.model as gm
    import gitcap.student as gs
    assert (gm.STOP_NEVER, gm.STOP_ALL_SEP) == (gs.STOP_NEVER, gs.STOP_ALL_SEP) == (s.STOP_NEVER, s.STOP_ALL_SEP) == (0, 1)
    assert gm.CaptionStream.push is gs.StudentCaptionStream.push is _WindowStream.push
