"""The restatement of the device frame samplers (tests/frame_sample_reference.py) against independent statements, and the
conditions the inputs of the GPU tests (tests/test_frame_sample_gpu.py, tests/test_frame_sample_e2e_gpu.py) must meet.  No GPU.

  features   torch.nn.functional.interpolate(mode="bilinear", align_corners=False) in fp64
  assign     a plain torch.cdist arg-min
  selection  the reference sampler's run-boundary loop (src/utils/frame_sampling_methods.py:186-192), re-stated on labels
  chain      gitcap.framegate.FrameGate's admit logic, fed with the restatement's distances
Each rule the device has to follow is shown to matter on these inputs: a restatement with a wrong tap, stride, tie rule,
empty-cluster rule or thinning formula misses."""
import numpy as np
import pytest
import torch

import frame_sample_reference as R
from frame_sample_reference import CHAIN_SHAPES, FEATURE_SHAPES, chain_video, selection_cases

# ---- features -------------------------------------------------------------------------------------------------------------------

def _video(N, H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (N, H, W, 3), dtype=np.uint8)


@pytest.mark.parametrize("size,out", FEATURE_SHAPES)
def test_features_equal_torch_bilinear(size, out):
    v = _video(3, *size, seed=size[0])
    got = R.features(v, *out).reshape(3, out[0], out[1], 3)
    want = torch.nn.functional.interpolate(torch.from_numpy(v).permute(0, 3, 1, 2).double(), size=out, mode="bilinear", align_corners=False)
    err = float((torch.from_numpy(got) - want.permute(0, 2, 3, 1)).abs().max())
    print(f"{size} -> {out}: max |restatement - torch| = {err:.3e}")
    assert err <= 1e-9                                     # both fp64: the coordinates differ in the last bits only
    if out == size:
        assert np.array_equal(got, v.astype(np.float64))   # the identity size is the identity


def test_a_wrong_tap_or_stride_misses_the_features_bound():
    v = _video(2, 37, 53, seed=3)
    good = R.features(v, 3, 5)
    shifted = R.features(np.roll(v, 1, axis=1), 3, 5)                         # every row tap one off
    transposed = R.features(v.transpose(0, 2, 1, 3), 5, 3).reshape(2, 5, 3, 3).transpose(0, 2, 1, 3).reshape(2, -1)
    assert np.abs(transposed - good).max() <= 1e-9                           # (the restatement treats rows and columns alike)
    wrong_stride = R.features(v.reshape(2, 53, 37, 3), 5, 3)                  # W taken for H
    for bad in (shifted, wrong_stride):
        assert np.abs(bad - good).max() > 1000 * R.FEATURES_BOUND
    assert R.FEATURES_BOUND < 1e-3


# ---- assign, update ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,D,k", [s for s in R.HOOK_SHAPES if s[1] <= 577 or s[0] <= 7])
def test_assign_equals_cdist_argmin_and_the_hook_inputs_have_margin(N, D, k):
    X, C = R.prototype_rows(N, D, k, seed=N + D + k)
    labels = R.assign(X, C)
    want = torch.cdist(torch.from_numpy(X).double(), torch.from_numpy(C).double()).argmin(1).numpy()
    assert np.array_equal(labels, want) and np.array_equal(labels, np.arange(N) % k)
    m = R.margins(X, C, m_max=N)
    assert int((m <= 0).sum()) == 0, (N, D, k, float(m.min()))


def test_the_largest_hook_inputs_have_margin():
    for N, D, k in [s for s in R.HOOK_SHAPES if s[1] > 577 and s[0] > 7]:
        X, C = R.prototype_rows(N, D, k, seed=N + D + k)
        d = R.sq_distances(X, C)
        assert np.array_equal(d.argmin(1), np.arange(N) % k)
        assert int((R.margins_of(d, D, m_max=N) <= 0).sum()) == 0, (N, D, k)


def test_ties_go_to_the_lower_cluster_and_the_rule_matters():
    X, C = R.prototype_rows(7, 45, 3, seed=1)
    C2 = np.concatenate([C[:2], C[1:2], C[2:]])             # cluster 2 is an exact copy of cluster 1
    labels = R.assign(X, C2)
    assert set(labels.tolist()) == {0, 1, 3}
    d = R.sq_distances(X, C2)
    last = d.shape[1] - 1 - d[:, ::-1].argmin(1)            # ties to the HIGHER cluster
    assert not np.array_equal(last, labels)


def test_update_is_the_mean_and_an_empty_cluster_keeps_its_centroid():
    X, C = R.prototype_rows(7, 64, 3, seed=2)
    labels = np.array([0, 2, 0, 2, 2, 0, 0])                # cluster 1 is empty
    new = R.update(X, labels, C)
    assert np.array_equal(new[1], C[1].astype(np.float64))
    for c in (0, 2):
        assert np.abs(new[c] - X[labels == c].astype(np.float64).mean(0)).max() <= 1e-12
    assert R.mean_bound(4, 256.0) < 1e-4


# ---- full k-means ---------------------------------------------------------------------------------------------------------------

def _relocating_kmeans(X, init, max_iter):
    """Lloyd with sklearn's empty-cluster rule in place of ours: an empty cluster moves to the row farthest from its centroid."""
    X = np.asarray(X, np.float64)
    C = X[np.asarray(init)].copy()
    labels = np.full(X.shape[0], -1)
    for it in range(1, max_iter + 1):
        d = R.sq_distances(X, C)
        new = d.argmin(1)
        if np.array_equal(new, labels):
            return labels, C, it
        labels = new
        C = R.update(X, labels, C)
        for c in range(C.shape[0]):
            if not (labels == c).any():
                C[c] = X[d.min(1).argmax()]
    return labels, C, max_iter


@pytest.mark.parametrize("name", sorted(R.KMEANS_VIDEOS))
def test_kmeans_inputs_have_margin_at_every_iteration(name):
    video, h2, w2, k, init, iters = R.kmeans_video(name)
    X = R.features(video, h2, w2)
    trace = []
    labels, C, got_iters = R.kmeans(X, init, 50, trace)
    assert got_iters == iters and len(trace) == iters
    exempt = 0
    for it, cent in trace:
        m = R.margins(X, cent, m_max=X.shape[0], x_err=R.FEATURES_BOUND)
        print(f"{name}: iteration {it}: smallest margin {float(m.min()):.3e}")
        exempt += int((m <= 0).sum())
    assert exempt == 0
    # stopping early gives what the full run had at that point; one iteration more changes nothing
    assert R.kmeans(X, init, iters)[2] == iters and np.array_equal(R.kmeans(X, init, iters)[0], labels)
    assert np.array_equal(R.kmeans(X, init, iters)[1], C)
    runs = R.KMEANS_VIDEOS[name][0]
    if name == "three runs":                               # the clusters are the prototypes
        assert len(set(zip(runs, labels.tolist()))) == 3
    if name == "changes sides":
        first = R.assign(X, trace[0][1])
        assert first[3] == 1 and labels[3] == 0            # the middle prototype went with the bright frames first
    if name == "empty cluster":
        assert set(labels.tolist()) == {0, 2} and np.array_equal(C[1], X[init[1]])
        other = _relocating_kmeans(X, init, 50)
        assert not np.array_equal(other[0], labels)        # sklearn's rule gives other labels here: the rule matters


# ---- selection ------------------------------------------------------------------------------------------------------------------

def _run_boundaries(classes):
    """the reference's loop (:186-192) on labels"""
    retained = [0]
    for i in range(1, len(classes)):
        if classes[i] != classes[i - 1]:
            retained.append(i)
    return retained


def test_selection_is_the_run_boundary_rule_and_thins():
    for N, labels, keep in selection_cases():
        full = R.select(N, N, keep=keep, labels=labels)
        assert full == (_run_boundaries(labels) if keep is None else [i for i in range(N) if keep[i]])
        K = len(full)
        for M in sorted({1, max(K - 1, 1), max(K, 1), K + 1}):
            got = R.select(N, M, keep=keep, labels=labels)
            assert len(got) == min(K, M) and got == sorted(set(got)) and set(got) <= set(full)
            if K > M:
                assert got[0] == full[0] and got == [full[int(np.floor(j * K / M))] for j in range(M)]
                if K >= 5 and M == K - 1:                  # another thinning formula picks other frames
                    assert got != [full[min(-(-j * K // M), K - 1)] for j in range(M)]


def test_host_samplers_follow_the_reference_arithmetic():
    from gitcap import sampling as S
    assert S.uniform_indices(100, 0.5) == list(range(0, 100, 2))
    assert S.uniform_indices(10, 0.35) == [0, 3, 6, 9]                           # int(3.5) = 3 retained -> interval 10 // 3
    g = torch.Generator().manual_seed(4)
    a = S.bin_indices(103, 10, g)
    assert len(a) == 10 and all(10 * b <= i < 10 * (b + 1) for b, i in enumerate(a))
    assert S.bin_indices(103, 10, torch.Generator().manual_seed(4)) == a
    assert S.bin_indices(3, 10, g) == []
    assert S.thin(list(range(10)), 4) == R.select(10, 4, keep=[1] * 10) == [0, 2, 5, 7]
    for N, k in ((18, 3), (15, 2), (300, 25), (7, 7)):
        assert S.default_init(N, k) == R.default_init(N, k)
    assert S.feature_size(480, 640, 0.1) == (48, 64)
    with pytest.raises(ValueError):
        S.feature_size(5, 5, 0.1)
    with pytest.raises(ValueError):
        S.sample_frames(torch.zeros((4, 8, 8, 3), dtype=torch.uint8), "nearest")
    with pytest.raises(ValueError):
        S.sample_frames(torch.zeros((4, 8, 8, 3), dtype=torch.uint8), "mse", num_bins=3)


# ---- chain ----------------------------------------------------------------------------------------------------------------------

class _FedGate:
    """FrameGate with its one device call replaced by the restatement's distances: what is left is the admit logic under test."""

    def __new__(cls, video, metric, threshold, channel, every):
        from gitcap.framegate import FrameGate
        gate = FrameGate(metric, threshold, channel, every)
        gate._distance = lambda frame, ref: R.G.distances(frame.numpy(), ref.numpy(), metric, channel)
        return gate


@pytest.mark.parametrize("H,W", CHAIN_SHAPES)
def test_chain_equals_the_gate_and_thresholds_sit_between_distances(H, W):
    for N in (1, 2, 9):
        video = chain_video(N, H, W)
        pairs = R.Pairs(video)
        for metric in ("mse", "hist"):
            for channel in (0, 2):
                thr = R.chain_thresholds(pairs, metric, channel)
                every_dist = pairs.all(metric, channel)
                if N == 9 and (H, W) != (1, 1):
                    assert "gap" in thr and "median" in thr
                for name, t in thr.items():
                    # no decision near a rounding edge: the threshold is a midpoint of neighbouring distinct distances (or beyond
                    # all of them), at least 1e-9 away, relatively, from every distance a chain can meet
                    for d in every_dist:
                        assert abs(d - t) >= 0.5e-9 * max(abs(d), abs(t)), (name, d, t)
                    if name in ("gap", "median"):
                        mids = dict(R.midpoint_thresholds(every_dist))
                        assert mids[t] >= 1e-9
                    for every in (1, 3):
                        keep, dist, refs = R.chain(pairs, metric, t, channel, every)
                        gate = _FedGate(video, metric, t, channel, every)
                        admitted = gate.admit(torch.from_numpy(video)[None])
                        assert admitted == [i for i in range(N) if keep[i]], (name, metric, channel, every)
                        assert all(keep[i] == 0 and dist[i] != dist[i] for i in range(N) if i % every)
                        if name == "all":
                            assert sum(keep) == len(range(0, N, every))
                        if name == "first":
                            assert sum(keep) == 1
                        if name == "gap" and N == 9 and every == 1 and (H, W) != (1, 1):
                            assert 1 < sum(keep) < N and any(r not in (-1, i - 1) for i, r in enumerate(refs))
