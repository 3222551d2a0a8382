"""Ragged batches, host side (gitcap/ragged.py): what `src` / `frame_counts` mean, their checks, the packing and the way back to
the reference's padded (visual_features, visual_features_valid) pair -- pure functions, no device -- and the C ABI's new symbols."""
import ctypes
import os
import re

import pytest
import torch

from gitcap import _lib, ragged

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 8           # image_size of these tests


def _padded(counts, fmax, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(len(counts), fmax, 3, S, S, generator=g)


def test_counts_are_validated():
    assert ragged.check_counts([1, 3, 2], 3, 3) == [1, 3, 2]
    assert ragged.check_counts(torch.tensor([2, 2], dtype=torch.int32), 2, 4) == [2, 2]
    for bad, B, limit in (([1, 0, 2], 3, 3), ([1, 4], 2, 3), ([1, 2], 3, 3), ([-1], 1, 3), ([1.5], 1, 3), ([True], 1, 3)):
        with pytest.raises(ValueError):
            ragged.check_counts(bad, B, limit)
    with pytest.raises(ValueError):
        ragged.check_counts(torch.tensor([1.0, 2.0]), 2, 3)
    with pytest.raises(ValueError):
        ragged.check_counts(torch.tensor([[1, 2]]), 2, 3)


def test_padded_and_list_forms_are_equivalent():
    counts = [1, 4, 3, 4, 2]
    x = _padded(counts, 4)
    x[1, 3:] += 0                                         # (a full clip)
    pa, ca, rawa = ragged.clips(x, counts, S, 6)
    lst = [x[b, :n].clone() for b, n in enumerate(counts)]
    pb, cb, rawb = ragged.clips(lst, None, S, 6)
    assert ca == cb == counts and rawa is rawb is False
    assert torch.equal(ragged.pack(pa), ragged.pack(pb))
    assert ragged.pack(pa).shape == (sum(counts), 3, S, S)
    # frames beyond a clip's count are ignored: poisoning them changes nothing
    y = x.clone()
    for b, n in enumerate(counts):
        y[b, n:] = float("nan")
    assert torch.equal(ragged.pack(ragged.clips(y, counts, S, 6)[0]), ragged.pack(pa))
    # clip-major: clip b's frames are adjacent, at offsets(counts)
    off = ragged.offsets(counts)
    assert off == [0, 1, 5, 8, 12] and ragged.offsets(counts, 17) == [17 * o for o in off]
    packed = ragged.pack(pa)
    for b, n in enumerate(counts):
        assert torch.equal(packed[off[b]:off[b] + n], x[b, :n])
    # the list's own counts win over nothing, and a disagreeing frame_counts is refused
    assert ragged.clips(lst, counts, S, 6)[1] == counts
    with pytest.raises(ValueError):
        ragged.clips(lst, [1, 4, 3, 4, 3], S, 6)


def test_uint8_camera_frames_and_shape_checks():
    counts = [2, 1]
    raw = torch.randint(0, 256, (2, 2, 12, 10, 3), dtype=torch.uint8)
    parts, c, is_raw = ragged.clips(raw, counts, S, 4)
    assert is_raw and c == counts and ragged.pack(parts).shape == (3, 12, 10, 3) and ragged.pack(parts).dtype == torch.uint8
    with pytest.raises(ValueError):                       # a padded tensor needs its counts
        ragged.clips(raw, None, S, 4)
    with pytest.raises(ValueError):                       # more frames than the padded tensor holds
        ragged.clips(raw, [3, 1], S, 4)
    with pytest.raises(ValueError):                       # above the handle's limit
        ragged.clips(_padded([3, 1], 3), [3, 1], S, 2)
    with pytest.raises(ValueError):                       # wrong image size
        ragged.clips(torch.zeros(2, 2, 3, S + 1, S + 1), [1, 2], S, 4)
    with pytest.raises(ValueError):                       # mixed dtypes
        ragged.clips([torch.zeros(1, 3, S, S), torch.zeros(2, 12, 10, 3, dtype=torch.uint8)], None, S, 4)
    with pytest.raises(ValueError):                       # an empty clip
        ragged.clips([torch.zeros(0, 3, S, S), torch.zeros(2, 3, S, S)], None, S, 4)
    with pytest.raises(ValueError):
        ragged.clips([], None, S, 4)


def test_equal_counts_are_the_dense_batch():
    x = _padded([3, 3], 4)
    parts, counts, _ = ragged.clips(x, [3, 3], S, 4)
    assert ragged.is_dense(counts) and not ragged.is_dense([3, 2])
    assert torch.equal(ragged.dense(parts), x[:, :3])


def test_unpack_rows_gives_the_padded_pair():
    counts, N, D = [2, 1, 3], 5, 4
    packed = torch.arange(sum(counts) * N * D, dtype=torch.float32).view(-1, D) + 1.0
    vis, valid = ragged.unpack_rows(packed, counts, N)
    assert vis.shape == (3, 3 * N, D) and valid.shape == (3, 3 * N) and valid.dtype == torch.bool
    at = 0
    for b, c in enumerate(counts):
        assert torch.equal(vis[b, :c * N], packed[at:at + c * N]) and bool((vis[b, c * N:] == 0).all())
        assert bool(valid[b, :c * N].all()) and not bool(valid[b, c * N:].any())
        at += c * N
    assert ragged.chunks([1] * 5, 2) == [(0, 2), (2, 4), (4, 5)]


def test_abi_has_the_ragged_symbols():
    names = ("gitcap_attach_frame_counts", "gitcap_dbg_attn_full_varlen", "gitcap_dbg_txt_block_varlen")
    hdr = open(os.path.join(ROOT, "include", "gitcap.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert os.path.exists(_lib.LIB_PATH), "build first: python -c 'import __graft_entry__ as g; g.build()'"
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for n in names:
        assert re.search(r"\b%s\s*\(" % n, hdr), n
        assert n in _lib.SYMBOLS and hasattr(lib, n), n
    blob = open(_lib.LIB_PATH, "rb").read()
    assert b"ragged_temporal_kernel" in blob and b"ragged_tables_kernel" in blob
    # a null handle is refused, not dereferenced
    lib.gitcap_attach_frame_counts.restype = ctypes.c_int
    lib.gitcap_attach_frame_counts.argtypes = [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.c_int]
    assert lib.gitcap_attach_frame_counts(None, (ctypes.c_int32 * 1)(1), 1) == -1
