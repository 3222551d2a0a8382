"""Measures, on the CPU, what fixes the bars of tests/test_tinyvit_gpu.py before any device run: for the inputs those
tests use, (a) the bf16-emulating reference with fp32 accumulation against the same rounding points with fp64
accumulation -- what a different summation order alone costs, per stage on its own (emulated) input -- and (b) the
emulating reference against the fp32 reference end to end (memory).  Unit: per row (one pixel's channel vector, one
frame's memory vector) max |d| / row RMS, and mean |d| / mean row RMS.

    python tools/tinyvit_tolerances.py
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-video-captioning_amd"), os.path.join(ROOT, "tests")]

from gitcap.tinyvit_config import tinyvit_config, tinyvit_synthetic_weights, tinyvit_tiny  # noqa: E402
from tinyvit_reference import TinyViTReference, make_frames, row_error  # noqa: E402

CASES = [("tiny", (2, 2, 2), 12, 7), ("tiny", (2, 2, 1), 12, 7), ("21m", (2, 2, 2), 6, 8), ("21m", (2, 2, 1), 6, 8)]


def main():
    torch.set_num_threads(min(16, os.cpu_count() or 1))
    worst = {"stem": [0, 0], "stage": [0, 0], "e2e": [0, 0]}
    for name, ms, n, seed in CASES:
        cfg = tinyvit_tiny(ms) if name == "tiny" else tinyvit_config("tiny_vit_21m_224", ms)
        w = tinyvit_synthetic_weights(cfg, 0)
        x = make_frames(n, cfg.img_size, seed)
        f32 = TinyViTReference(cfg).load_weights(w)
        e32 = TinyViTReference(cfg, True).load_weights(w)
        e64 = TinyViTReference(cfg, True, torch.float64).load_weights(w)
        prev = e32.stem(x)
        r = row_error(prev, e64.stem(x.double()))
        print(f"{name} {ms} stem order {r[0]:.4f} {r[1]:.5f}")
        worst["stem"] = [max(a, b) for a, b in zip(worst["stem"], r)]
        for i in range(4):
            o32, o64 = e32.stage(i, prev), e64.stage(i, prev.double())
            r = row_error(o32, o64)
            print(f"{name} {ms} stage {i} order {r[0]:.4f} {r[1]:.5f}")
            worst["stage"] = [max(a, b) for a, b in zip(worst["stage"], r)]
            prev = o32
        m_f32 = f32.memory(x.view(1, n, *x.shape[1:]))[0]
        m_e32 = prev.mean(dim=[2, 3])
        m_e64 = e64.memory(x.double().view(1, n, *x.shape[1:]))[0]
        a, b = row_error(m_e32, m_f32), row_error(m_e32, m_e64)
        e2e = [a[0] + b[0], a[1] + b[1]]
        print(f"{name} {ms} memory: emulated vs fp32 {a[0]:.4f} {a[1]:.5f}; order {b[0]:.4f} {b[1]:.5f}")
        worst["e2e"] = [max(p, q) for p, q in zip(worst["e2e"], e2e)]
    print("worst (max-row, mean):", {k: [round(v, 5) for v in vals] for k, vals in worst.items()})


if __name__ == "__main__":
    main()
