"""Per-caption wall time of the student's live loop (the reference's src/real_time_inference.py: TinyViT-21M encoder + 2-layer
decoder, six frames per caption), B = 1, 480x640 uint8 camera frames already on the device, 25 greedy tokens, stop = never:
  (a) full    = gitcap_preprocess of the last six frames + greedy_decode(frames): every caption encodes six frames
  (b) stream  = caption_stream(hop=1).push(one raw frame): encodes the new frame only (gitcap_tinyvit_encode_raw), pushes its
                memory token (gitcap_student_window_push) and captions the window (gitcap_student_window_greedy)
Host clock around a device synchronise, warmed up, the series interleaved update by update as a1, b, a2: (a) is timed twice per
update so that the difference of its two medians gives the run-to-run spread a difference between (a) and (b) has to exceed.
Every update also checks that the two captions are equal.

Usage: python tools/student_live.py [out.txt]
       python tools/student_live.py --only a|b --iters K    (no timing, K updates of one form: for launch counts under
                                                             rocprofv3 --kernel-trace --stats; count(2K) - count(K) = K updates)"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "real-time-video-captioning_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from gitcap.preprocess import preprocess_frames  # noqa: E402
from gitcap.student import StudentCaptioner  # noqa: E402
from gitcap.student_config import student_base, student_synthetic_weights  # noqa: E402
from gitcap.tinyvit_config import tinyvit_config, tinyvit_synthetic_weights  # noqa: E402

NAME = "tiny_vit_21m_224.dist_in22k_ft_in1k"
H, W, MAX_LEN, WARMUP = 480, 640, 25, 10


def build():
    scfg, tcfg = student_base(), tinyvit_config(NAME)
    weights = dict(student_synthetic_weights(scfg, 0))
    weights.update({"image_encoder.model." + k: v for k, v in tinyvit_synthetic_weights(tcfg, 0).items()})
    return StudentCaptioner(NAME, cfg=scfg, weights=weights, image_encoder="native", device="cuda:0", max_batch=1,
                            max_text_len=MAX_LEN, stop="never")


def fmt(xs):
    q = statistics.quantiles(xs, n=4)
    return f"{statistics.median(xs):7.3f} [q1 {q[0]:.3f} .. q3 {q[2]:.3f}; min {min(xs):.3f}, max {max(xs):.3f}]"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("out", nargs="?")
    ap.add_argument("--only", choices=("a", "b"))
    ap.add_argument("--iters", type=int, default=int(os.environ.get("ITERS", "60")))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/student_live.py measures on the GPU; no HIP device is visible")
    m = build()
    F = m.cfg.mem_tokens
    total = F + (0 if args.only else WARMUP) + args.iters
    pool = torch.randint(0, 256, (1, total, H, W, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).cuda()

    def full(k):                                   # (a): the parent's way on frames k-5 .. k
        return m.greedy_decode(preprocess_frames(pool[:, k + 1 - F:k + 1]), max_len=MAX_LEN, stop="never")

    st = m.caption_stream(hop=1, max_len=MAX_LEN, stop="never")
    assert st.push(pool[:, :F - 1]) is None        # the first five frames: the window is one frame short
    torch.cuda.synchronize()
    if args.only:
        for k in range(F - 1, total - 1):
            out = full(k) if args.only == "a" else st.push(pool[:, k])
        torch.cuda.synchronize()
        print(f"{args.iters} updates of form ({args.only}); last caption {out[0, :8].tolist()} ...")
        return
    ta1, tb, ta2 = [], [], []
    for k in range(F - 1, total - 1):
        stamps = []
        for fn in (lambda: full(k), lambda: st.push(pool[:, k]), lambda: full(k)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            stamps.append(((time.perf_counter() - t0) * 1e3, out))
        assert torch.equal(stamps[0][1], stamps[1][1]) and torch.equal(stamps[0][1], stamps[2][1]), "captions differ"
        if k >= F - 1 + WARMUP:
            ta1.append(stamps[0][0]); tb.append(stamps[1][0]); ta2.append(stamps[2][0])
    ma1, mb, ma2 = statistics.median(ta1), statistics.median(tb), statistics.median(ta2)
    ma, spread = statistics.median(ta1 + ta2), abs(ma1 - ma2)
    lines = [f"student live loop: TinyViT-21M + student_base, B = 1, {H}x{W} uint8 frames on the device, {MAX_LEN} greedy tokens "
             f"(stop=never); host clock around torch.cuda.synchronize(), {WARMUP} warm-up + {len(tb)} interleaved updates "
             f"(a1, b, a2), ms: median [quartiles; range]",
             f"(a1) preprocess 6 frames + greedy_decode(frames)   {fmt(ta1)}",
             f"(a2) the same, second series                       {fmt(ta2)}",
             f"(b)  caption_stream(hop=1).push(1 raw frame)       {fmt(tb)}",
             f"(a) both series: median {ma:.3f} ms; spread of (a) = |median a1 - median a2| = {spread:.3f} ms",
             f"(b) - (a) = {mb - ma:+.3f} ms; (b) / (a) = {mb / ma:.3f}; condition (b) <= (a) + spread: "
             f"{'met' if mb <= ma + spread else 'NOT MET'}; captions equal on every update"]
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
