"""The device frame samplers (csrc/framesample.hip: gitcap_frame_chain, gitcap_frame_features, gitcap_kmeans and its two hooks,
gitcap_frame_select) against the numpy restatement (tests/frame_sample_reference.py).

  chain      keep and the implied reference sequence exact; dist as tests/test_frame_gate_gpu.py holds gitcap_frame_change
             (relative 1e-12, 0 exactly 0), and bit for bit what gitcap_frame_change gives for the same pairs
  features   within FEATURES_BOUND (derived in the restatement file from the fp32 rounding points)
  assign     labels exact on inputs whose fp64 margins exceed the assign bound (tests/test_frame_sample.py checks them)
  update     within mean_bound; bitwise repeatable; an empty cluster keeps its centroid
  k-means    labels, iters and selected indices equal the restatement's on the prototype videos
  selection  exact"""
import numpy as np
import pytest
import torch

import frame_sample_reference as R
from gpu_support import assert_tail, lib, poisoned, ptr, same_bits, stream, to_dev  # noqa: F401
from frame_sample_reference import CHAIN_SHAPES, FEATURE_SHAPES, chain_video, selection_cases

pytestmark = pytest.mark.gpu

ERR_ARG = -1
REL = 1e-12
I32, I64, U8, F32, F64 = torch.int32, torch.int64, torch.uint8, torch.float32, torch.float64


def _near(got, want):
    return abs(got - want) <= REL * abs(want)          # want == 0: got must be exactly 0


# ---- chain ----------------------------------------------------------------------------------------------------------------------

def _chain(lib, video, metric, channel, thr, every):
    """video: device uint8 [N,H,W,3] (any alignment) -> keep [N], dist [N] on the host; the words behind both stay poisoned"""
    N, H, W = video.shape[:3]
    keep, dist = poisoned(N + 16, 77, U8), poisoned(N + 4, -7.5, F64)
    assert lib.gitcap_frame_chain(ptr(video), N, H, W, int(metric == "hist"), channel, thr, every, ptr(keep), ptr(dist), stream()) == 0
    assert_tail(keep, N, 77)
    assert_tail(dist, N, -7.5)
    return keep[:N].tolist(), dist[:N].tolist()


@pytest.mark.parametrize("N", [1, 2, 9])
@pytest.mark.parametrize("H,W", CHAIN_SHAPES)
def test_chain_equals_the_restatement_and_the_pair_calls(lib, H, W, N):
    from gitcap.framegate import frame_change
    video = chain_video(N, H, W)
    pairs = R.Pairs(video)
    n = video.size
    ran = 0
    for off in (0, 1, 7):                                  # the video at a byte offset inside a larger buffer
        buf = torch.zeros(n + 64, dtype=U8, device="cuda")
        assert buf.data_ptr() % 16 == 0
        dev = buf[off:off + n].view(N, H, W, 3)
        dev.copy_(torch.from_numpy(video))
        for metric in ("mse", "hist"):
            for channel in (0, 2):
                for name, thr in R.chain_thresholds(pairs, metric, channel).items():
                    for every in (1, 3):
                        what = f"{N}x{H}x{W} offset {off} {metric} channel {channel} threshold {name} every {every}"
                        want_keep, want_dist, refs = R.chain(pairs, metric, thr, channel, every)
                        keep, dist = _chain(lib, dev, metric, channel, thr, every)
                        assert keep == want_keep, (what, keep, want_keep)
                        assert dist[0] != dist[0]
                        for i in range(1, N):
                            if refs[i] < 0:
                                assert dist[i] != dist[i], (what, i)
                                continue
                            assert _near(dist[i], want_dist[i]), (what, i, dist[i], want_dist[i])
                            if every == 1 or off == 1:     # the same pair through gitcap_frame_change, at the same addresses: bit for bit
                                key = "mse" if metric == "mse" else "chisq"
                                one = frame_change(dev[i:i + 1], dev[refs[i]:refs[i] + 1], channel, outputs=(key,))[key]
                                assert dev[i:i + 1].data_ptr() == dev.data_ptr() + i * H * W * 3
                                assert np.float64(one.item()).tobytes() == np.float64(dist[i]).tobytes(), (what, i)
                        ran += 1
    assert ran >= 3 * 2 * 2 * 2 * 2


# ---- features -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("size,out", FEATURE_SHAPES)
def test_features_within_the_derived_bound(lib, size, out):
    N = 3
    video = np.random.default_rng(size[0] + out[0]).integers(0, 256, (N, *size, 3), dtype=np.uint8)
    D = out[0] * out[1] * 3
    X = poisoned(N * D + 16, float("nan"))
    assert lib.gitcap_frame_features(ptr(to_dev(video, U8)), N, size[0], size[1], out[0], out[1], ptr(X), stream()) == 0
    assert_tail(X, N * D, float("nan"))
    got = X[:N * D].view(N, D).double().cpu().numpy()
    err = float(np.abs(got - R.features(video, *out)).max())
    print(f"{size} -> {out}: max |device - fp64| = {err:.3e}, bound {R.FEATURES_BOUND:.3e}")
    assert err <= R.FEATURES_BOUND
    if out == size:
        assert np.array_equal(got, video.reshape(N, -1).astype(np.float64))


# ---- assign, update -------------------------------------------------------------------------------------------------------------

def _assign(lib, X, C, labels_in=None):
    N, D = X.shape
    labels = poisoned(N + 16, -1, I32)
    if labels_in is not None:
        labels[:N] = to_dev(labels_in, I32)
    changed = torch.zeros(1, dtype=I32, device="cuda")
    assert lib.gitcap_dbg_kmeans_assign(ptr(X), N, D, C.shape[0], ptr(C), ptr(labels), ptr(changed), stream()) == 0
    assert_tail(labels, N, -1)
    return labels[:N].cpu().numpy(), int(changed.item())


def _update(lib, X, labels, C):
    N, D = X.shape
    k = C.shape[0]
    out = poisoned(k * D + 16, float("nan"))
    out[:k * D] = C.reshape(-1)
    assert lib.gitcap_dbg_kmeans_update(ptr(X), N, D, k, ptr(to_dev(labels, I32)), ptr(out), stream()) == 0
    assert_tail(out, k * D, float("nan"))
    return out[:k * D].view(k, D).clone()


@pytest.mark.parametrize("N,D,k", R.HOOK_SHAPES)
def test_assign_and_update_hooks(lib, N, D, k):
    Xn, Cn = R.prototype_rows(N, D, k, seed=N + D + k)
    X, C = to_dev(Xn, F32), to_dev(Cn, F32)
    want = np.arange(N) % k                                # tests/test_frame_sample.py: the restatement's labels, with margin
    labels, changed = _assign(lib, X, C)
    assert np.array_equal(labels, want) and changed == N
    again, changed = _assign(lib, X, C, labels_in=labels)
    assert np.array_equal(again, want) and changed == 0
    if N > 1:
        flipped = labels.copy()
        flipped[::2] = k                                   # any other value counts as a change
        assert _assign(lib, X, C, labels_in=flipped)[1] == (N + 1) // 2

    new = _update(lib, X, want, C)
    ref = R.update(Xn, want, Cn)
    m = -(-N // k)
    err = float(np.abs(new.double().cpu().numpy() - ref).max())
    bound = R.mean_bound(m, 256.0)
    print(f"N={N} D={D} k={k}: max |centroid - fp64| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound
    assert same_bits(_update(lib, X, want, C), new)
    if k >= 3:                                             # cluster 1 loses its rows to cluster 0: it keeps its centroid
        moved = np.where(want == 1, 0, want)
        kept = _update(lib, X, moved, C)
        assert same_bits(kept[1], C[1]) and not same_bits(kept[0], new[0])
        assert float(np.abs(kept.double().cpu().numpy() - R.update(Xn, moved, Cn)).max()) <= R.mean_bound(2 * m, 256.0)


def test_ties_between_duplicate_centroids_go_to_the_lower_index(lib):
    for N, D, k in ((7, 45, 3), (300, 577, 3), (7, 9216, 3)):
        Xn, Cn = R.prototype_rows(N, D, k, seed=1)
        for dup_at in (1, 3, 4, 5):                        # inside a tile of four centroids and across its edge
            C2 = np.concatenate([Cn, Cn, Cn[:1]])          # 7 centroids
            C2[dup_at] = C2[0]
            want = R.assign(Xn, C2)
            assert not (want == dup_at).any()
            got, _ = _assign(lib, to_dev(Xn, F32), to_dev(C2, F32))
            assert np.array_equal(got, want), (N, D, dup_at)


# ---- full k-means ---------------------------------------------------------------------------------------------------------------

def _kmeans(lib, X, k, init, max_iter):
    N, D = X.shape
    labels, cent, iters = poisoned(N + 16, -9, I32), poisoned(k * D + 16, float("nan")), poisoned(1 + 16, -9, I32)
    assert lib.gitcap_kmeans(ptr(X), N, D, k, ptr(to_dev(init, I32)), max_iter, ptr(labels), ptr(cent), ptr(iters), stream()) == 0
    assert_tail(labels, N, -9)
    assert_tail(cent, k * D, float("nan"))
    assert_tail(iters, 1, -9)
    return labels[:N].cpu().numpy(), cent[:k * D].view(k, D).clone(), int(iters[0].item())


@pytest.mark.parametrize("name", sorted(R.KMEANS_VIDEOS))
def test_kmeans_equals_the_restatement_on_the_prototype_videos(lib, name):
    from gitcap.sampling import sample_frames
    video, h2, w2, k, init, iters = R.kmeans_video(name)
    N, H, W = video.shape[:3]
    ratio = R.KMEANS_VIDEOS[name][2]
    want_labels, want_cent, want_iters = R.kmeans(R.features(video, h2, w2), init, 50)
    assert want_iters == iters
    X = torch.empty((N, h2 * w2 * 3), dtype=F32, device="cuda")
    assert lib.gitcap_frame_features(ptr(to_dev(video, U8)), N, H, W, h2, w2, ptr(X), stream()) == 0
    labels, cent, got_iters = _kmeans(lib, X, k, init, 50)
    assert np.array_equal(labels, want_labels) and got_iters == iters
    bound = R.mean_bound(N, 256.0) + R.FEATURES_BOUND
    assert float(np.abs(cent.double().cpu().numpy() - want_cent).max()) <= bound
    # converged at `iters` of 50: the same labels and centroids, bit for bit, as a run that is only given `iters` iterations
    short = _kmeans(lib, X, k, init, iters)
    assert np.array_equal(short[0], labels) and short[2] == iters and same_bits(short[1], cent)
    assert same_bits(_kmeans(lib, X, k, init, 50)[1], cent)
    if iters > 1:                                          # one iteration fewer: cut off, and reported so
        cut = _kmeans(lib, X, k, init, iters - 1)
        assert cut[2] == iters - 1
    # the sampler: features, k-means and selection in one call, thinned and not
    for max_frames in (None, 3):
        sel = sample_frames(torch.from_numpy(video), "cluster", max_frames=max_frames, num_classes=k, downsampling_ratio=ratio,
                            max_iter=50, init=list(init))
        want = R.select(N, N if max_frames is None else max_frames, labels=want_labels)
        assert sel.indices[0].tolist() == want and sel.counts == [len(want)]
        assert sel.labels[0].tolist() == want_labels.tolist() and int(sel.iters[0].item()) == iters
        assert same_bits(sel.centroids[0], cent)
        assert torch.equal(sel.frames()[0].cpu(), torch.from_numpy(video[want]))


# ---- selection ------------------------------------------------------------------------------------------------------------------

def test_selection_equals_the_restatement(lib):
    ran = 0
    for N, labels, keep in selection_cases():
        K = len(R.select(N, N, keep=keep, labels=labels))
        for M in sorted({1, max(K - 1, 1), max(K, 1), K + 1}):
            want = R.select(N, M, keep=keep, labels=labels)
            idx, count = poisoned(N + 16, -3, I64), poisoned(1 + 16, -3, I32)
            rc = lib.gitcap_frame_select(ptr(to_dev(keep, U8)), ptr(to_dev(labels, I32)), N, M, ptr(idx), ptr(count), stream())
            assert rc == 0
            assert_tail(idx, N, -3)
            assert_tail(count, 1, -3)
            assert int(count[0].item()) == len(want) and idx[:len(want)].tolist() == want, (N, M)
            assert bool((idx[len(want):N] == -1).all())
            ran += 1
    assert ran >= 3 * 6 * 2


# ---- bad arguments --------------------------------------------------------------------------------------------------------------

def test_bad_arguments_are_refused_before_any_launch(lib):
    N, H, W, k, D = 4, 6, 5, 2, 9
    st = stream()
    video = to_dev(np.zeros((N, H, W, 3), np.uint8), U8)
    X, init = torch.zeros((N, D), device="cuda"), to_dev([0, 1], I32)
    keep, dist = poisoned(N, 77, U8), poisoned(N, -7.5, F64)
    feat, labels, cent = poisoned(N * D, -7.5), poisoned(N, -9, I32), poisoned(k * D, -7.5)
    iters, idx, count, changed = poisoned(1, -9, I32), poisoned(N, -3, I64), poisoned(1, -9, I32), poisoned(1, -9, I32)
    v, x, i0, kp, ds, ft, lb, ce, it, ix, cn, ch = (ptr(t) for t in (video, X, init, keep, dist, feat, labels, cent, iters, idx, count, changed))
    chain = lambda *a: lib.gitcap_frame_chain(*a, st)
    bad = [chain(None, N, H, W, 0, 2, 1.0, 1, kp, ds), chain(v, N, H, W, 0, 2, 1.0, 1, None, ds), chain(v, N, H, W, 0, 2, 1.0, 1, kp, None),
           chain(v, 0, H, W, 0, 2, 1.0, 1, kp, ds), chain(v, -1, H, W, 0, 2, 1.0, 1, kp, ds), chain(v, N, 0, W, 0, 2, 1.0, 1, kp, ds),
           chain(v, N, H, 0, 0, 2, 1.0, 1, kp, ds), chain(v, N, H, W, 2, 2, 1.0, 1, kp, ds), chain(v, N, H, W, -1, 2, 1.0, 1, kp, ds),
           chain(v, N, H, W, 0, 3, 1.0, 1, kp, ds), chain(v, N, H, W, 0, -1, 1.0, 1, kp, ds), chain(v, N, H, W, 0, 2, 1.0, 0, kp, ds)]
    features = lambda *a: lib.gitcap_frame_features(*a, st)
    bad += [features(None, N, H, W, 1, 3, ft), features(v, N, H, W, 1, 3, None), features(v, 0, H, W, 1, 3, ft), features(v, N, 0, W, 1, 3, ft),
            features(v, N, H, W, 0, 3, ft), features(v, N, H, W, 1, 0, ft), features(v, N, H, W, -1, 3, ft)]
    kmeans = lambda *a: lib.gitcap_kmeans(*a, st)
    bad += [kmeans(None, N, D, k, i0, 5, lb, ce, it), kmeans(x, N, D, k, None, 5, lb, ce, it), kmeans(x, N, D, k, i0, 5, None, ce, it),
            kmeans(x, N, D, k, i0, 5, lb, None, it), kmeans(x, N, D, k, i0, 5, lb, ce, None), kmeans(x, 0, D, k, i0, 5, lb, ce, it),
            kmeans(x, N, 0, k, i0, 5, lb, ce, it), kmeans(x, N, D, 0, i0, 5, lb, ce, it), kmeans(x, N, D, N + 1, i0, 5, lb, ce, it),
            kmeans(x, N, D, k, i0, 0, lb, ce, it)]
    bad += [lib.gitcap_dbg_kmeans_assign(x, N, D, 0, ce, lb, ch, st), lib.gitcap_dbg_kmeans_assign(x, N, D, N + 1, ce, lb, ch, st),
            lib.gitcap_dbg_kmeans_assign(x, N, D, k, None, lb, ch, st), lib.gitcap_dbg_kmeans_assign(x, N, D, k, ce, lb, None, st),
            lib.gitcap_dbg_kmeans_update(x, N, D, 0, lb, ce, st), lib.gitcap_dbg_kmeans_update(x, N, D, N + 1, lb, ce, st),
            lib.gitcap_dbg_kmeans_update(x, N, D, k, None, ce, st), lib.gitcap_dbg_kmeans_update(None, N, D, k, lb, ce, st)]
    select = lambda *a: lib.gitcap_frame_select(*a, st)
    bad += [select(None, None, N, 2, ix, cn), select(kp, None, 0, 2, ix, cn), select(kp, None, N, 0, ix, cn), select(kp, None, N, -1, ix, cn),
            select(kp, None, N, 2, None, cn), select(kp, None, N, 2, ix, None)]
    assert bad == [ERR_ARG] * len(bad) and len(bad) == 12 + 7 + 10 + 8 + 6
    torch.cuda.synchronize()
    for t, fill in ((keep, 77), (dist, -7.5), (feat, -7.5), (labels, -9), (cent, -7.5), (iters, -9), (idx, -3), (count, -9), (changed, -9)):
        assert_tail(t, 0, fill)
    assert lib.gitcap_abi_version() == 1
