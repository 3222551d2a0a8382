"""The two kernels of the teacher's stream pool through their debug hooks (include/gitcap.h: gitcap_dbg_pool_scatter,
gitcap_dbg_pool_assemble), bit for bit: the scatter against the numpy restatement, the assemble against the window's and the
ragged path's own kernels on the same rows (gitcap_dbg_window_assemble, gitcap_dbg_ragged_temporal).  The inputs are those
tests/test_teacher_pool.py shows to tell wrong kernels apart.  Sizes: D below one wave's 256 columns and D = 768 (three passes of
the column loop), 3 rows per frame, so 15 and 21 rows: no multiple of the 4 rows of a block, more than one block."""
import ctypes

import numpy as np
import pytest
import torch

import teacher_pool_reference as R
from gpu_support import NAN, assert_tail, bf16_bits, lib, poisoned, ptr, same_bits, stream, to_dev  # noqa: F401

pytestmark = pytest.mark.gpu

ERR_ARG = -1
N = 3
FRAMES = R.GPU_S * R.GPU_F


def _ring(D, seed):
    return np.random.default_rng(seed).standard_normal((FRAMES, N, D)).astype(np.float32)


@pytest.mark.parametrize("D", [64, 768])
def test_pool_scatter_writes_the_planned_ring_frames_and_nothing_else(lib, D):
    p = R.gpu_pool()
    dst = p.push(R.GPU_PUSH)                                            # five frames, mixed order, stream 1 across the wrap
    assert len(dst) * N % 4 != 0
    stage = np.random.default_rng(2).standard_normal((len(dst), N, D)).astype(np.float32)
    ring = poisoned(FRAMES * N * D + 16, NAN)
    stage_t, dst_t = to_dev(stage, torch.float32), to_dev(dst, torch.int32)
    assert lib.gitcap_dbg_pool_scatter(ptr(stage_t), ptr(ring), FRAMES, ptr(dst_t), len(dst), N, D, stream()) == 0
    torch.cuda.synchronize()
    want = R.scatter(np.full((FRAMES, N, D), np.nan, np.float32), stage, dst)
    assert same_bits(ring[:FRAMES * N * D], to_dev(want.reshape(-1), torch.float32))          # NaN poison included: the 4 other frames
    assert_tail(ring, FRAMES * N * D, NAN)


def test_pool_scatter_refuses_bad_arguments_before_any_launch(lib):
    D = 64
    stage, ring = to_dev(np.zeros((2, N, D), np.float32), torch.float32), poisoned(FRAMES * N * D, NAN)
    ok, high, low, twice = (to_dev(v, torch.int32) for v in ([4, 1], [4, FRAMES], [-1, 2], [4, 4]))       # (held until the calls are over)
    bad = [(ptr(stage), ptr(ring), FRAMES, ptr(high), 2, N, D),                                   # a ring frame out of range
           (ptr(stage), ptr(ring), FRAMES, ptr(low), 2, N, D),
           (ptr(stage), ptr(ring), FRAMES, ptr(twice), 2, N, D),                                  # two writers of one frame
           (ptr(stage), ptr(ring), FRAMES, ptr(ok), 2, N, D + 2),                                 # D % 4
           (ptr(stage), ptr(ring), FRAMES, ptr(ok), 0, N, D), (ptr(stage), ptr(ring), FRAMES, ptr(ok), 2, 0, D),
           (None, ptr(ring), FRAMES, ptr(ok), 2, N, D), (ptr(stage), None, FRAMES, ptr(ok), 2, N, D), (ptr(stage), ptr(ring), FRAMES, None, 2, N, D),
           (ctypes.c_void_p(stage.data_ptr() + 4), ptr(ring), FRAMES, ptr(ok), 2, N, D)]
    for args in bad:
        assert lib.gitcap_dbg_pool_scatter(*args, stream()) == ERR_ARG, args[2:]
    torch.cuda.synchronize()
    assert bool(torch.isnan(ring).all())


def _assemble(lib, ring_t, temporal_t, trows, src, pos, D, rows_cap):
    out = poisoned(rows_cap * D + 16, NAN, torch.bfloat16)
    src_t, pos_t = to_dev(src, torch.int32), to_dev(pos, torch.int32)
    rc = lib.gitcap_dbg_pool_assemble(ptr(ring_t), FRAMES, ptr(temporal_t), trows, ptr(src_t), ptr(pos_t), ptr(out), len(src), N, D, stream())
    torch.cuda.synchronize()
    assert rc == 0
    assert_tail(out, len(src) * N * D, NAN)                              # rows behind the packed total keep their poison
    return out[:len(src) * N * D]


@pytest.mark.parametrize("D", [64, 768])
@pytest.mark.parametrize("head", [0, 2])
def test_pool_assemble_on_a_lockstep_state_is_window_assemble(lib, D, head):
    B, F = R.GPU_S, R.GPU_F
    p = R.Pool(B, F)
    for _ in range(F + head):                                           # every stream full, its next slot = head: a lockstep window
        p.push(list(range(B)))
    src, pos, _, ln, out3 = p.call(list(range(B)))
    assert p.heads() == [head] * B and out3 == (B * F, F, 1)
    ring = _ring(D, 3)
    temporal = np.random.default_rng(4).standard_normal((F, D)).astype(np.float32)
    ring_t, temporal_t = to_dev(ring, torch.float32), to_dev(temporal, torch.float32)
    for tt, tn in ((temporal_t, temporal), (None, None)):               # with and without a temporal table
        got = _assemble(lib, ring_t, tt, F if tt is not None else 0, src, pos, D, B * F * N + 5)
        want = poisoned(B * F * N * D + 16, NAN, torch.bfloat16)
        assert lib.gitcap_dbg_window_assemble(ptr(ring_t), ptr(tt), ptr(want), None, B, F, head, N, D, stream()) == 0
        torch.cuda.synchronize()
        assert same_bits(got, want[:B * F * N * D])
        assert np.array_equal(bf16_bits(got), R.bf16_round(R.assemble(ring, tn, src, pos)).reshape(-1))


@pytest.mark.parametrize("D", [64, 768])
def test_pool_assemble_on_a_ragged_plan_is_ragged_temporal_on_the_packed_rows(lib, D):
    p = R.gpu_pool()
    p.push(R.GPU_PUSH)
    src, pos, off, ln, out3 = p.call([1, 2, 0])
    assert ln == [3, 2, 2] and out3 == (7, 3, 0) and 7 * N % 4 != 0
    ring = _ring(D, 5)
    temporal = np.random.default_rng(6).standard_normal((R.GPU_F, D)).astype(np.float32)
    ring_t, temporal_t = to_dev(ring, torch.float32), to_dev(temporal, torch.float32)
    packed = to_dev(ring[src].reshape(-1, D), torch.float32)           # the same rows laid out packed
    got = _assemble(lib, ring_t, temporal_t, R.GPU_F, src, pos, D, 7 * N + 3)
    want = poisoned(7 * N * D + 16, NAN, torch.bfloat16)
    pos_t = to_dev(pos, torch.int32)
    assert lib.gitcap_dbg_ragged_temporal(ptr(packed), ptr(temporal_t), R.GPU_F, ptr(pos_t), ptr(want), None, 7, N, D, stream()) == 0
    torch.cuda.synchronize()
    assert same_bits(got, want[:7 * N * D])
    assert np.array_equal(bf16_bits(got), R.bf16_round(R.assemble(ring, temporal, src, pos)).reshape(-1))
    # without a temporal table: the rows' own bf16 rounding (pos is not read)
    bare = _assemble(lib, ring_t, None, 0, src, pos, D, 7 * N + 3)
    assert same_bits(bare, packed.bfloat16().reshape(-1))
    assert np.array_equal(bf16_bits(bare), R.bf16_round(R.assemble(ring, None, src, pos)).reshape(-1))


def test_pool_assemble_refuses_bad_arguments_before_any_launch(lib):
    D = 64
    ring_t = to_dev(_ring(D, 7), torch.float32)
    temporal_t = to_dev(np.zeros((R.GPU_F, D), np.float32), torch.float32)
    out = poisoned(2 * N * D, NAN, torch.bfloat16)
    held = []                                                           # the tables live until the calls are over

    def t(v):
        held.append(to_dev(v, torch.int32))
        return ptr(held[-1])
    bad = [(ptr(ring_t), FRAMES, ptr(temporal_t), R.GPU_F, t([0, FRAMES]), t([0, 1]), ptr(out), 2, N, D),     # src out of range
           (ptr(ring_t), FRAMES, ptr(temporal_t), R.GPU_F, t([0, -1]), t([0, 1]), ptr(out), 2, N, D),
           (ptr(ring_t), FRAMES, ptr(temporal_t), R.GPU_F, t([0, 1]), t([0, R.GPU_F]), ptr(out), 2, N, D),    # pos beyond the table
           (ptr(ring_t), FRAMES, ptr(temporal_t), R.GPU_F, t([0, 1]), None, ptr(out), 2, N, D),
           (ptr(ring_t), FRAMES, ptr(temporal_t), R.GPU_F, t([0, 1]), t([0, 1]), ptr(out), 2, N, D + 2),
           (ptr(ring_t), FRAMES, ptr(temporal_t), R.GPU_F, t([0, 1]), t([0, 1]), ptr(out), 2, N, 1028),
           (ptr(ring_t), FRAMES, ptr(temporal_t), R.GPU_F, t([0, 1]), t([0, 1]), ptr(out), 0, N, D),
           (None, FRAMES, ptr(temporal_t), R.GPU_F, t([0, 1]), t([0, 1]), ptr(out), 2, N, D),
           (ptr(ring_t), FRAMES, ptr(temporal_t), R.GPU_F, t([0, 1]), t([0, 1]), None, 2, N, D)]
    for args in bad:
        assert lib.gitcap_dbg_pool_assemble(*args, stream()) == ERR_ARG, args[1:]
    torch.cuda.synchronize()
    assert bool(torch.isnan(out.float()).all())
