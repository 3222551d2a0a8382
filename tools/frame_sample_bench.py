#!/usr/bin/env python3
"""What sampling whole videos on the device costs, against the ways there were before (profiles/r23_frame_sampling.txt).

    python tools/frame_sample_bench.py [--videos 1 16] [--frames 300] [--reps 5]

Videos of `--frames` 480x640 uint8 frames on the device: 25 random prototype frames in runs of 12, every byte with noise in
[-2, 2].  GIT-base (synthetic weights) with 6 frames per clip, 20 tokens, stop = never.  In one process, after a warm-up, p50 of
`--reps` repetitions, HIP-event and wall time (wall includes the synchronisation), for one video and for 16:
  (a) chain      sample_frames(videos, "mse", threshold=100): gitcap_frame_chain + gitcap_frame_select, one copy of B counts
  (b) gate       the same frames pushed one by one through FrameGate.admit: a launch, a copy of one double and a host decision
                 per frame -- the only way there was, and what (a) is measured against
  (c) cluster    sample_frames(videos, "cluster", num_classes=25, downsampling_ratio=0.1): features, Lloyd, selection
  (d) torch      the same Lloyd loop in torch device ops (interpolate, cdist arg-min, index_add_ means, the changed count read
                 on the host every iteration)
  (e) captions   caption_videos(model, videos, "mse", threshold=100, max_len=20) end to end
The selections of (a) / (b) and the labels of (c) / (d) are compared, so the numbers are for equal work."""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "real-time-video-captioning_amd")):
    sys.path.insert(0, p)

import torch  # noqa: E402


def timed(fn, n, warm):
    """p50 (event ms, wall ms) of n calls of fn() after `warm` unrecorded ones; each call is followed by a synchronisation."""
    ev, wall = [], []
    for i in range(warm + n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        if i >= warm:
            ev.append(a.elapsed_time(b))
            wall.append((t1 - t0) * 1e3)
    return statistics.median(ev), statistics.median(wall)


def make_video(frames, seed):
    g = torch.Generator(device="cuda").manual_seed(seed)
    protos = torch.randint(0, 256, (25, 480, 640, 3), dtype=torch.int16, device="cuda", generator=g)
    out = torch.empty((frames, 480, 640, 3), dtype=torch.uint8, device="cuda")
    for t in range(frames):
        noise = torch.randint(-2, 3, (480, 640, 3), dtype=torch.int16, device="cuda", generator=g)
        out[t] = (protos[(t // 12) % 25] + noise).clamp_(0, 255).to(torch.uint8)
    return out


def torch_lloyd(video, k, ratio, max_iter):
    """The cluster sampler in torch device ops, the same rules: bilinear features, direct distances, ordered means, the empty
    cluster keeps its centroid, stop at the first iteration that changes no label (read on the host)."""
    N, H, W = video.shape[:3]
    h2, w2 = int(H * ratio), int(W * ratio)
    X = torch.nn.functional.interpolate(video.permute(0, 3, 1, 2).float(), size=(h2, w2), mode="bilinear", align_corners=False)
    X = X.permute(0, 2, 3, 1).reshape(N, -1).contiguous()
    C = X[torch.tensor([(2 * j + 1) * N // (2 * k) for j in range(k)], device=X.device)].clone()
    labels = torch.full((N,), -1, dtype=torch.int64, device=X.device)
    for it in range(1, max_iter + 1):
        new = torch.cdist(X, C, compute_mode="donot_use_mm_for_euclid_dist").argmin(1)
        changed = int((new != labels).sum().item())
        labels = new
        if changed == 0:
            break
        sums = torch.zeros_like(C).index_add_(0, labels, X)
        cnt = torch.bincount(labels, minlength=k).to(X.dtype)[:, None]
        C = torch.where(cnt > 0, sums / cnt.clamp(min=1), C)
    return labels, it


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--videos", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--frames", type=int, default=300)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    args = ap.parse_args()

    from gitcap.config import git_base
    from gitcap.framegate import FrameGate
    from gitcap.model import GitCaptioner
    from gitcap.sampling import caption_videos, sample_frames
    from gitcap.weights import synthetic_weights

    cfg = git_base(6)
    m = GitCaptioner(cfg, synthetic_weights(cfg, seed=0), device="cuda:0", max_batch=16, max_frames=6, max_text_len=20, stop="never")
    pool = [make_video(args.frames, s) for s in range(max(args.videos))]
    rows = []
    for B in args.videos:
        vids = pool[:B]
        sel = sample_frames(vids, "mse", threshold=100.0)
        gate_sel = []
        for v in vids:
            gate_sel.append(FrameGate("mse", 100.0).admit(v[None]))
        assert [i.tolist() for i in sel.indices] == gate_sel, "chain and gate disagree"
        cl = sample_frames(vids, "cluster", num_classes=25, downsampling_ratio=0.1)
        tl = [torch_lloyd(v, 25, 0.1, 100) for v in vids]
        agree = [bool((a == b[0].int()).all()) for a, b in zip(cl.labels, tl)]
        iters = [int(i.item()) for i in cl.iters]

        def gate_all():
            for v in vids:
                FrameGate("mse", 100.0).admit(v[None])

        r = {"videos": B, "frames": args.frames, "kept_chain": sel.counts, "kept_cluster": cl.counts, "kmeans_iters": iters,
             "torch_iters": [b[1] for b in tl], "labels_equal_torch": agree}
        r["chain"] = timed(lambda: sample_frames(vids, "mse", threshold=100.0), args.reps, args.warmup)
        r["gate"] = timed(gate_all, args.reps, args.warmup)
        r["cluster"] = timed(lambda: sample_frames(vids, "cluster", num_classes=25, downsampling_ratio=0.1), args.reps, args.warmup)
        r["torch"] = timed(lambda: [torch_lloyd(v, 25, 0.1, 100) for v in vids], args.reps, args.warmup)
        r["captions"] = timed(lambda: caption_videos(m, vids, "mse", max_len=20, stop="never", threshold=100.0), args.reps, args.warmup)
        rows.append(r)
        print(f"{B} video(s) of {args.frames} frames: kept by the chain {sel.counts[:4]}..., by the clusters {cl.counts[:4]}..., "
              f"k-means iterations {iters[:4]}... (torch {r['torch_iters'][:4]}...), labels equal torch's: {all(agree)}")
        for key, what in (("chain", "(a) chain"), ("gate", "(b) gate, frame by frame"), ("cluster", "(c) cluster"),
                          ("torch", "(d) torch Lloyd"), ("captions", "(e) caption_videos")):
            print(f"    {what:28s} p50 of {args.reps}: {r[key][0]:9.3f} ms HIP events / {r[key][1]:9.3f} ms wall", flush=True)
    print(json.dumps(rows))


if __name__ == "__main__":
    main()
