"""Restatement of the device frame samplers in numpy fp64 / Python ints, written from the definitions (include/gitcap.h:
gitcap_frame_chain, gitcap_frame_features, gitcap_kmeans, gitcap_frame_select; gitcap/sampling.py), for tests/test_frame_sample.py,
tests/test_frame_sample_gpu.py and tests/test_frame_sample_e2e_gpu.py.  The pair distances of the chain are
tests/frame_gate_reference.py's.

The bounds the GPU tests hold the device to are derived here from the roundings the device's fp32 arithmetic makes (u = 2^-24, the
unit roundoff: fl(x) = x (1 + e), |e| <= u), not measured.

FEATURES_BOUND.  The taps and the remainders that make the weights are integers, hence exact.  A weight l = fl(rem / den) has
absolute error <= u (l < 1); its complement fl(1 - l) another <= u on top, so <= 2u.  A weight product w = fl(wy wx) of two such
weights <= 1: <= 2u + 2u + u = 5u (first order).  A term fl(v w), v <= 255 exact: <= 255 (5u + u) = 1530 u.  Four terms: 6120 u.
Three additions of partial sums that stay <= 255 (1 + small): <= 3 * 255 u = 765 u.  Total 6885 u = 27 * 255 u; the second-order
terms and the (1 + small) are far below the one unit of 255 u added: FEATURES_BOUND = 28 * 255 * u = 4.3e-4 (the values are up
to 255, a wrong tap or weight is off by whole grey levels).

assign_bound.  A computed distance sum_d fl(fl(x_d - c_d)^2), D terms added in any order: every term carries (1 + e)^3 (one
subtraction, one product -- the subtraction's rounding counted twice) and at most D - 1 additions, so |computed - d| <=
(D + 2) u d to first order; (D + 3) u d is used.  The device's centroids are fp32 means, the restatement's fp64: an element is
off by at most eps_c = mean_bound(m, 255) for a cluster of m rows, so the centroid by at most sqrt(D) eps_c in norm and the
distance by 2 sqrt(d) sqrt(D) eps_c + D eps_c^2.  Two candidates' order is certain when their fp64 distances differ by more than
the sum of their two bounds: the "margin" the CPU tests check for every frame at every iteration.

mean_bound.  m values |x| <= xmax added in ascending order in fp32: <= (m - 1) u * (m xmax) on the sum, / m -> (m - 1) u xmax;
the division adds u xmax: m u xmax; (m + 1) u xmax is used."""
import math

import numpy as np

import frame_gate_reference as G

U = 2.0 ** -24
FEATURES_BOUND = 28 * 255 * U
NAN = float("nan")


# ---- gate chain -----------------------------------------------------------------------------------------------------------------

class Pairs:
    """The pair distances of one video, computed once each: pairs(i, ref, metric, channel)."""

    def __init__(self, video):
        self.video, self.memo = np.asarray(video), {}

    def __call__(self, i, ref, metric, channel):
        key = (i, ref, metric, 0 if metric == "mse" else channel)
        if key not in self.memo:
            self.memo[key] = G.distances(self.video[i][None], self.video[ref][None], metric, channel)[0]
        return self.memo[key]

    def all(self, metric, channel):
        """every distance a chain over this video can meet: frame i against any earlier frame"""
        N = self.video.shape[0]
        return [self(i, r, metric, channel) for i in range(N) for r in range(i)]


def chain(video, metric, threshold, channel=2, every=1):
    """video uint8 [N,H,W,3] (or a Pairs of it) -> (keep [N] of 0/1, dist [N] floats (NaN: frame 0 and frames not looked at),
    refs [N]: the frame each looked-at frame was compared with, -1 otherwise)."""
    pairs = video if isinstance(video, Pairs) else Pairs(video)
    N = pairs.video.shape[0]
    keep, dist, refs = [0] * N, [NAN] * N, [-1] * N
    keep[0] = 1
    ref = 0
    for i in range(every, N, every):
        dist[i] = pairs(i, ref, metric, channel)
        refs[i] = ref
        if dist[i] > threshold:
            keep[i] = 1
            ref = i
    return keep, dist, refs


# ---- features -------------------------------------------------------------------------------------------------------------------

def _taps(n_in, n_out):
    """per output position: (tap 0, tap 1, weight of tap 1) from the exact quotient ((2i + 1) n_in - n_out) / (2 n_out), not below 0"""
    out = []
    for i in range(n_out):
        num = max((2 * i + 1) * n_in - n_out, 0)
        q, r = divmod(num, 2 * n_out)
        out.append((q, min(q + 1, n_in - 1), r / (2.0 * n_out)))
    return out


def features(video, h2, w2):
    """video uint8 [N,H,W,3] -> fp64 [N, h2*w2*3] (order y, x, channel): bilinear, half-pixel centres."""
    v = np.asarray(video).astype(np.float64)
    N, H, W, _ = v.shape
    ty, tx = _taps(H, h2), _taps(W, w2)
    out = np.empty((N, h2, w2, 3), np.float64)
    for y, (y0, y1, ly) in enumerate(ty):
        for x, (x0, x1, lx) in enumerate(tx):
            out[:, y, x] = (v[:, y0, x0] * ((1 - ly) * (1 - lx)) + v[:, y0, x1] * ((1 - ly) * lx)
                            + v[:, y1, x0] * (ly * (1 - lx)) + v[:, y1, x1] * (ly * lx))
    return out.reshape(N, -1)


# ---- k-means --------------------------------------------------------------------------------------------------------------------

def sq_distances(X, C):
    """fp64 [N, k]: sum_d (x_d - c_d)^2, the direct difference."""
    X, C = np.asarray(X, np.float64), np.asarray(C, np.float64)
    out = np.empty((X.shape[0], C.shape[0]), np.float64)
    for c in range(C.shape[0]):                             # a centroid at a time: [N, k, D] at once would not fit for k = N = 300
        diff = X - C[c]
        out[:, c] = np.einsum("nd,nd->n", diff, diff)
    return out


def assign(X, C):
    """labels int64 [N]: the arg-min over c, ties to the lower c (numpy's argmin takes the first)."""
    return sq_distances(X, C).argmin(1)


def update(X, labels, C):
    """new centroids fp64 [k, D]: the mean of each cluster's rows; a cluster without rows keeps its row of C."""
    X, labels = np.asarray(X, np.float64), np.asarray(labels)
    out = np.array(C, np.float64, copy=True)
    for c in range(out.shape[0]):
        rows = X[labels == c]
        if len(rows):
            out[c] = rows.sum(0) / len(rows)
    return out


def mean_bound(m, xmax):
    return (m + 1) * U * xmax


def assign_bound(d, D, m_max, x_err=0.0, xmax=255.0):
    """How far the device's fp32 distance (to its fp32 centroid) may be from the fp64 distance d (module docstring).  x_err: how far
    an element of the device's X may be from the restatement's (FEATURES_BOUND when X comes from gitcap_frame_features, 0 when both
    sides are given the same fp32 rows): the row moves by x_err, the centroid -- a mean of such rows -- by x_err more."""
    eps = mean_bound(m_max, xmax) + 2.0 * x_err
    return (D + 3) * U * d + 2.0 * np.sqrt(d * D) * eps + D * eps * eps


def margins(X, C, m_max, x_err=0.0):
    """Per frame: (d2 - d1) - (bound(d1) + bound(d2)) for the nearest and second-nearest DISTINCT centroid; > 0 = the label is
    certain (exact duplicates of a centroid give the device exactly equal distances: the tie rule, not a margin).  One distinct
    centroid: +inf."""
    return margins_of(sq_distances(X, np.unique(np.asarray(C, np.float64), axis=0)), np.asarray(X).shape[1], m_max, x_err)


def margins_of(d, D, m_max, x_err=0.0):
    """margins from the distances [N, k] to distinct centroids"""
    d = np.sort(d, 1)
    if d.shape[1] < 2:
        return np.full(d.shape[0], np.inf)
    return (d[:, 1] - d[:, 0]) - (assign_bound(d[:, 0], D, m_max, x_err) + assign_bound(d[:, 1], D, m_max, x_err))


def kmeans(X, init_idx, max_iter, trace=None):
    """Lloyd with the device's rules -> (labels [N], centroids fp64 [k, D], iters).  The first iteration whose assign changes no
    label is the last (its update is not run); iters = its number, or max_iter.  trace (a list): gets (iteration, centroids
    the assign used) appended."""
    X = np.asarray(X, np.float64)
    C = X[np.asarray(init_idx)].copy()
    labels = np.full(X.shape[0], -1)
    for it in range(1, max_iter + 1):
        if trace is not None:
            trace.append((it, C.copy()))
        new = assign(X, C)
        changed = int((new != labels).sum())
        labels = new
        if changed == 0:
            return labels, C, it
        C = update(X, labels, C)
    return labels, C, max_iter


def default_init(N, k):
    return [math.floor((j + 0.5) * N / k) for j in range(k)]


# ---- selection ------------------------------------------------------------------------------------------------------------------

def select(N, max_frames, keep=None, labels=None):
    """-> the selected indices (ascending).  keep: flags; else labels: 0 and every run boundary.  Thinned to
    kept[floor(j K / max_frames)] when K > max_frames."""
    if keep is not None:
        kept = [i for i in range(N) if keep[i]]
    else:
        kept = [i for i in range(N) if i == 0 or labels[i] != labels[i - 1]]
    K = len(kept)
    if K > max_frames:
        kept = [kept[(j * K) // max_frames] for j in range(max_frames)]
    return kept


# ---- the samplers end to end ------------------------------------------------------------------------------------------------------

def sample_chain(video, metric, threshold, max_frames, channel=2, every=1):
    keep, _, _ = chain(video, metric, threshold, channel, every)
    return select(len(keep), max_frames, keep=keep)


def sample_cluster(video, k, ratio, max_frames, max_iter=100):
    video = np.asarray(video)
    N, H, W = video.shape[:3]
    X = features(video, int(H * ratio), int(W * ratio))
    labels, _, iters = kmeans(X, default_init(N, k), max_iter)
    return select(N, max_frames, labels=labels), labels, iters


# ---- inputs ---------------------------------------------------------------------------------------------------------------------

def prototype_video(runs, H, W, seed, noise=2, levels=None):
    """uint8 [N,H,W,3]: frame t shows prototype runs[t] (a random frame per prototype, each in its own brightness band: 60 wide
    from a level of its own, or 30 wide from levels[p]) plus per-frame noise in [-noise, noise] on every byte: frames of a
    prototype are near each other and far from the others."""
    rng = np.random.default_rng(seed)
    protos = {}
    for p in sorted(set(runs)):
        lo, width = (20 + (37 * p) % 160, 60) if levels is None else (levels[p], 30)
        protos[p] = rng.integers(lo, lo + width, (H, W, 3)).astype(np.int64)
    out = np.empty((len(runs), H, W, 3), np.uint8)
    for t, p in enumerate(runs):
        out[t] = np.clip(protos[p] + rng.integers(-noise, noise + 1, (H, W, 3)), 0, 255).astype(np.uint8)
    return out


def midpoint_thresholds(dists):
    """The distinct finite distances, sorted -> the midpoints between neighbours, with the relative gap of each:
    [(threshold, (hi - lo) / hi)]."""
    vals = sorted({d for d in dists if d == d})
    return [((lo + hi) / 2.0, (hi - lo) / hi) for lo, hi in zip(vals, vals[1:])]


def chain_thresholds(pairs, metric, channel):
    """The thresholds the chain tests use on one video -> {name: threshold}.  "all": below every distance (they are >= 0);
    "first": the largest value the metric can take, which > never exceeds (mse <= 255^2; chi-square: a term is (hr - hf)^2 / hr <=
    hr + hf^2, so the sum is <= P + P^2 for P pixels); "gap" / "median": the midpoint of the widest relative gap / the middle gap
    between neighbouring distinct distances of any two frames (absent when all distances are equal).  A midpoint of ALL pair
    distances is off every distance any chain can meet, whatever frames the chain keeps."""
    H, W = pairs.video.shape[1:3]
    out = {"all": -1.0, "first": 65025.0 if metric == "mse" else float(H * W + (H * W) ** 2)}
    mids = midpoint_thresholds(pairs.all(metric, channel))
    if mids:
        out["gap"] = max(mids, key=lambda m: m[1])[0]
        out["median"] = mids[len(mids) // 2][0]
    return out


def prototype_rows(N, D, k, seed):
    """fp32 X [N, D], C [k, D]: k random centroids in [0, 255), row n = centroid n % k plus noise in [-1, 1)."""
    rng = np.random.default_rng(seed)
    C = rng.uniform(0, 255, (k, D)).astype(np.float32)
    X = (C[np.arange(N) % k] + rng.uniform(-1, 1, (N, D))).astype(np.float32)
    return X, C


HOOK_SHAPES = [(N, D, k) for D in (45, 64, 577, 9216) for N in (1, 7, 300) for k in sorted({1, min(3, N), N})]

# the prototype videos of the full k-means tests: name -> (runs, (H, W), ratio, k, levels, init or None (the default rows), iters)
KMEANS_VIDEOS = {
    # the default rows 3, 9, 15 fall into three different prototypes: assigned once, confirmed once
    "three runs": ([0] * 4 + [1] * 3 + [2] * 5 + [0] * 2 + [1] * 4, (37, 53), 0.2, 3, {0: 30, 1: 120, 2: 200}, None, 2),
    # two clusters for three prototypes at levels 40, 100, 200: the middle one first goes with the many bright frames, whose mean
    # (175) is then farther from it than the dark centroid: it changes sides in iteration 2
    "changes sides": ([0] * 3 + [1] * 3 + [2] * 9, (61, 47), 0.1, 2, {0: 40, 1: 100, 2: 200}, [0, 3], 3),
    # two initial centroids on the same row, the only frame of its prototype: the tie goes to the lower cluster, whose mean stays
    # that row exactly, so the higher one stays empty and keeps its centroid
    "empty cluster": ([0] + [1] * 6 + [2] * 5, (37, 53), 0.2, 3, {0: 30, 1: 120, 2: 200}, [0, 0, 8], 2),
    # alternating prototypes: every frame is a run boundary; 40 selected frames
    "alternating": ([0, 1] * 20, (20, 30), 0.5, 2, {0: 50, 1: 180}, [0, 1], 2),
}


def kmeans_video(name):
    """-> (video uint8, h2, w2, k, init rows, expected iters)"""
    runs, (H, W), ratio, k, levels, init, iters = KMEANS_VIDEOS[name]
    video = prototype_video(runs, H, W, 1000 + len(runs), noise=2, levels=levels)
    return video, int(H * ratio), int(W * ratio), k, (default_init(len(runs), k) if init is None else init), iters


# ---- shapes and inputs the CPU and the GPU tests share -----------------------------------------------------------------------------

CHAIN_SHAPES = [(1, 1), (37, 53), (61, 47), (120, 160)]
CHAIN_RUNS = [0, 0, 1, 1, 1, 2, 0, 0, 3]


def chain_video(N, H, W):
    """the video of the chain tests: near-repeats inside a run, another prototype at a run boundary"""
    return prototype_video(CHAIN_RUNS[:N], H, W, 7 * H + W + N)


FEATURE_SHAPES = [((37, 53), (3, 5)), ((120, 160), (12, 16)), ((5, 5), (1, 1)), ((37, 53), (37, 53))]


def selection_cases():
    """(N, labels, keep) of the selection tests: all kept, one kept, alternating labels, runs; N across the workgroup size"""
    out = []
    for N in (1, 2, 1100):
        rng = np.random.default_rng(N)
        out.append((N, np.arange(N) % 7, None))                                   # all kept (every label differs from the last)
        out.append((N, np.zeros(N, np.int64), None))                              # one kept
        out.append((N, np.arange(N) % 2, None))                                   # alternating
        out.append((N, np.repeat(rng.integers(0, 5, N // 3 + 1), 3)[:N], None))   # runs
        out.append((N, None, (rng.integers(0, 3, N) == 0).astype(np.uint8)))      # flags; frame 0 may be dropped
        out.append((N, None, np.ones(N, np.uint8)))
    return out
