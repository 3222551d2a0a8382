"""Student captioner from frames (SURVEY par. 8 f.2): latency of the native TinyViT-21m encoder alone and of
frames -> 25-token greedy caption, at the webcam shape (B = 1 clip of F = 6 frames, src/real_time_inference.py) and at
B = 16, against the test reference module (tests/tinyvit_reference.py) run in torch eager bf16 on the same device.
Medians of ITERS timed calls after warmup (cuda events around each call).

    python tools/student_encoder_latency.py [merge strides, e.g. 2,2,1]
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-video-captioning_amd"), os.path.join(ROOT, "tests")]

from gitcap.student import StudentCaptioner  # noqa: E402
from gitcap.student_config import student_base, student_synthetic_weights  # noqa: E402
from gitcap.tinyvit_config import tinyvit_config, tinyvit_synthetic_weights  # noqa: E402
from tinyvit_reference import TinyViTReference, make_frames  # noqa: E402

ITERS = int(os.environ.get("ITERS", "30"))


def gflop_per_frame(cfg) -> float:
    """Multiply-adds x 2 of every conv, Linear and attention product (LayerNorm, GELU, softmax not counted)."""
    C, maps, img = cfg.embed_dims, cfg.stage_maps(), cfg.img_size
    f = 2 * (img // 2) ** 2 * (C[0] // 2) * 27 + 2 * maps[0] ** 2 * C[0] * (C[0] // 2) * 9
    hw = maps[0] ** 2
    f += cfg.depths[0] * (2 * hw * C[0] * 4 * C[0] * 2 + 2 * hw * 4 * C[0] * 9)
    for i in range(1, 4):
        hwp, hw, c, n = maps[i - 1] ** 2, maps[i] ** 2, C[i], cfg.window_sizes[i] ** 2
        f += 2 * hwp * C[i - 1] * c + 2 * hw * c * 9 + 2 * hw * c * c
        f += cfg.depths[i] * (2 * hw * c * 3 * c + 4 * hw * n * c + 2 * hw * c * c + 2 * hw * c * 9 + 2 * hw * c * 4 * c * 2)
    return f / 1e9


def p50(fn):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(ITERS):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    ts.sort()
    return ts[len(ts) // 2]


def main():
    ms = tuple(int(v) for v in sys.argv[1].split(",")) if len(sys.argv) > 1 else (2, 2, 2)
    tcfg, scfg = tinyvit_config("tiny_vit_21m_224", ms), student_base()
    tw, sw = tinyvit_synthetic_weights(tcfg, 0), student_synthetic_weights(scfg, 0)
    weights = dict(sw)
    weights.update({"image_encoder.model." + k: v for k, v in tw.items()})
    m = StudentCaptioner("tiny_vit_21m_224", cfg=scfg, weights=weights, image_encoder="native", max_batch=16, max_text_len=25)
    enc = m.image_encoder
    eager = TinyViTReference(tcfg, dtype=torch.bfloat16).load_weights(tw).to(device="cuda", dtype=torch.bfloat16)
    gf = gflop_per_frame(tcfg)
    print(f"TinyViT-21m, merge strides {ms}: {gf:.2f} GFLOP per frame (convs, Linears, attention products)")
    for B in (1, 16):
        x = make_frames(B * 6, 224, 1).view(B, 6, 3, 224, 224).cuda()
        with torch.no_grad():
            t_enc = p50(lambda: enc.memory(x))
            t_cap = p50(lambda: m.greedy_decode(x, max_len=25, stop="never"))
            t_eager = p50(lambda: eager(x.view(B * 6, 3, 224, 224).to(torch.bfloat16))[-1].float().mean(dim=[2, 3]))
            eager_mem = eager(x.view(B * 6, 3, 224, 224).to(torch.bfloat16))[-1].float().mean(dim=[2, 3]).view(B, 6, -1)
            t_eager_cap = p50(lambda: m.greedy_decode(
                eager(x.view(B * 6, 3, 224, 224).to(torch.bfloat16))[-1].float().mean(dim=[2, 3]).view(B, 6, -1),
                max_len=25, stop="never"))
        tflops = gf * B * 6 / (t_enc * 1e-3) / 1e3
        print(f"B={B:2d} F=6 ({B * 6} frames): encoder p50 {t_enc:.3f} ms ({tflops:.1f} TFLOP/s = {100 * tflops / 2500:.2f}% of "
              f"2.5 PF bf16) | frames -> 25-token caption p50 {t_cap:.3f} ms | eager-torch bf16 encoder {t_eager:.3f} ms, "
              f"eager encoder + native decoder caption {t_eager_cap:.3f} ms | eager memory rms "
              f"{float(eager_mem.pow(2).mean().sqrt()):.3f}", flush=True)


if __name__ == "__main__":
    main()
