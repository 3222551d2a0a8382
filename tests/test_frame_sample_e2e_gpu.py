"""Decoded videos to captions with no host decision in between (gitcap/sampling.py: caption_videos): the captions of three synthetic
videos of different length and frame size equal, bit for bit, greedy_decode on the frames the restatement
(tests/frame_sample_reference.py) selects, each clip alone -- the path the parity tests hold to the goldens."""
import pytest
import torch

import frame_sample_reference as R
from gpu_support import captioner_cls  # noqa: F401

pytestmark = pytest.mark.gpu

MAX_LEN = 8
LEVELS = {0: 30, 1: 120, 2: 200}
# runs of three prototypes; the default initial rows floor((j + 0.5) N / 3) fall into three different prototypes
RUNS = ([0] * 4 + [1] * 4 + [2] * 4,                                                       # 3 run boundaries
        [0, 0, 1, 0, 1, 0, 0, 0, 1, 1, 1, 1, 0, 1, 0, 2, 2, 2, 0, 2],                      # 12: thinned to the frame limit of 8
        [0, 0, 1, 0, 1, 1, 2, 2, 0])                                                       # 6
SIZES = ((40, 48), (37, 53), (60, 80))
THRESHOLD = {"mse": 100.0, "hist": 500.0}
RATIO, K = 0.2, 3


@pytest.fixture(scope="module")
def setup(captioner_cls):
    from gitcap.config import git_tiny
    from gitcap.weights import synthetic_weights
    cfg = git_tiny(num_frames=8)
    m = captioner_cls(cfg, synthetic_weights(cfg, seed=0), device="cuda:0", max_batch=3, max_frames=8, max_text_len=12)
    videos = [R.prototype_video(runs, H, W, 50 + i, noise=2, levels=LEVELS) for i, (runs, (H, W)) in enumerate(zip(RUNS, SIZES))]
    alone = {}

    def caption(b, idx):
        """greedy_decode of video b's frames `idx`, the clip alone; computed once per selection"""
        key = (b, tuple(idx))
        if key not in alone:
            alone[key] = m.greedy_decode(torch.from_numpy(videos[b][list(idx)])[None].cuda(), max_len=MAX_LEN, stop="never")
        return alone[key]
    return m, videos, caption


def _check(m, videos, caption, method, want, **kw):
    from gitcap.sampling import caption_videos
    ids, sel = caption_videos(m, [torch.from_numpy(v) for v in videos], method, max_len=MAX_LEN, stop="never", **kw)
    assert sel.counts == [len(w) for w in want] and max(sel.counts) <= m._frame_limit()
    assert [i.tolist() for i in sel.indices] == want, (method, [i.tolist() for i in sel.indices], want)
    assert ids.shape == (len(videos), MAX_LEN + 1)
    for b, w in enumerate(want):
        assert torch.equal(ids[b:b + 1].cpu(), caption(b, w).cpu()), (method, b)
    return sel


@pytest.mark.parametrize("metric", ["mse", "hist"])
def test_chain_captions_equal_greedy_on_the_restatements_frames(setup, metric):
    m, videos, caption = setup
    thr = THRESHOLD[metric]
    want = []
    for v in videos:
        keep, dist, _ = R.chain(v, metric, thr)
        # no decision near a rounding edge: every distance is at most half the threshold or at least twice it
        assert all(d != d or d <= thr / 2 or d >= 2 * thr for d in dist), (metric, dist)
        want.append(R.select(len(keep), 8, keep=keep))
    assert len({len(w) for w in want}) > 1 and any(sum(R.chain(v, metric, thr)[0]) > 8 for v in videos)     # ragged, and one is thinned
    sel = _check(m, videos, caption, metric, want, threshold=thr)
    for v, d in zip(videos, sel.distances):
        ref = R.chain(v, metric, thr)[1]
        got = d.tolist()
        assert all((a != a and b != b) or abs(a - b) <= 1e-12 * abs(b) for a, b in zip(got, ref))
    # every third frame only
    want3 = [R.sample_chain(v, metric, thr, 8, every=3) for v in videos]
    _check(m, videos, caption, metric, want3, threshold=thr, every=3)


def test_cluster_captions_equal_greedy_on_the_restatements_frames(setup):
    m, videos, caption = setup
    want, labels = [], []
    for v, runs in zip(videos, RUNS):
        idx, lab, iters = R.sample_cluster(v, K, RATIO, 8)
        assert iters == 2 and len(set(zip(runs, lab.tolist()))) == 3          # the clusters are the prototypes
        H, W = v.shape[1:3]
        X = R.features(v, int(H * RATIO), int(W * RATIO))
        trace = []
        R.kmeans(X, R.default_init(len(runs), K), 100, trace)
        assert all((R.margins(X, c, len(runs), R.FEATURES_BOUND) > 0).all() for _, c in trace)
        want.append(idx)
        labels.append(lab.tolist())
    assert [len(w) for w in want] == [3, 8, 6]
    sel = _check(m, videos, caption, "cluster", want, num_classes=K, downsampling_ratio=RATIO)
    assert [l.tolist() for l in sel.labels] == labels and [int(i.item()) for i in sel.iters] == [2, 2, 2]


def test_a_selection_is_a_ragged_list_for_the_other_calls(setup):
    from gitcap.sampling import sample_frames
    m, videos, caption = setup
    pair = [videos[0], videos[0][:8]]                      # one frame size (a batch shares its frame shape), 3 and 2 frames kept
    sel = sample_frames([torch.from_numpy(v) for v in pair], "mse", max_frames=m._frame_limit(), threshold=THRESHOLD["mse"])
    want = [R.sample_chain(v, "mse", THRESHOLD["mse"], 8) for v in pair]
    assert [i.tolist() for i in sel.indices] == want and sel.counts == [3, 2]
    vis, valid = m.forward_image_enc(sel.frames())
    assert valid.sum(1).tolist() == [c * m.cfg.tokens_per_frame for c in sel.counts]
    y = torch.cat([caption(0, w) for w in want], 0)
    got = m.score(sel.frames(), y)
    for b, w in enumerate(want):
        one = m.score(torch.from_numpy(videos[0][w])[None].cuda(), y[b:b + 1])
        assert torch.equal(got["token_logprobs"][b:b + 1].cpu(), one["token_logprobs"].cpu())
    assert m.infer(sel.frames(), beam_size=1, max_steps=MAX_LEN)["predictions"].shape[0] == 2


def test_uniform_and_bins_return_the_host_arithmetic(setup):
    from gitcap.sampling import caption_videos, sample_frames
    m, videos, caption = setup
    limit = m._frame_limit()
    vids = [torch.from_numpy(v) for v in videos]
    thin = lambda kept: kept if len(kept) <= limit else [kept[j * len(kept) // limit] for j in range(limit)]
    want = []
    for v in videos:
        N = v.shape[0]
        interval = N // int(N * 0.5)                        # the reference's arithmetic (:62-70)
        want.append(thin([i for i in range(N) if i % interval == 0]))
    _check(m, videos, caption, "uniform", want, retention_rate=0.5)
    a = sample_frames(vids, "bins", max_frames=limit, num_bins=4, seed=7)
    b = sample_frames(vids, "bins", max_frames=limit, num_bins=4, seed=7)
    c = sample_frames(vids, "bins", max_frames=limit, num_bins=4, seed=8)
    assert [i.tolist() for i in a.indices] == [i.tolist() for i in b.indices] != [i.tolist() for i in c.indices]
    g = torch.Generator().manual_seed(7)
    for v, idx in zip(videos, a.indices):
        per = v.shape[0] // 4
        draws = torch.randint(0, per, (4,), generator=g).tolist()
        assert idx.tolist() == [q * per + d for q, d in enumerate(draws)] and idx.device.type == "cuda"
    ids, sel = caption_videos(m, vids, "bins", max_len=MAX_LEN, stop="never", num_bins=4, seed=7)
    assert sel.counts == [4, 4, 4] and ids.shape == (3, MAX_LEN + 1)
    for bb, idx in enumerate(a.indices):
        assert torch.equal(ids[bb:bb + 1].cpu(), caption(bb, idx.tolist()).cpu())
