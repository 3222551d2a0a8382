"""Latency of the student's search that ends hypotheses at SEP (StudentCaptioner.beam_search(eos=True)) against the plain search,
and of a pool call with beams against the cameras captioned one by one: base student with synthetic weights, memory pushed,
k = 3, max_len = 25, p50 of 5 timed calls behind 2 warm-up calls.  Also reports, per search case, how many of the max_len - 1 steps
ran after every clip was done (from beam_search_host's statistics): what an early exit of the loop would save.
Prints one JSON line; the alternating `bench.py` comparison with the parent build is a separate, manual step."""
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "real-time-video-captioning_amd")]

import torch  # noqa: E402

K, MAX_LEN, CAMERAS, CLIPS = 3, 25, 16, 4


def p50_ms(fn, warmup=2, reps=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return round(statistics.median(out), 3)


def main():
    from gitcap.student import StudentCaptioner
    from gitcap.student_config import student_base, student_synthetic_weights
    cfg = student_base()
    m = StudentCaptioner(cfg=cfg, weights=student_synthetic_weights(cfg, 0), device="cuda:0", max_batch=CAMERAS * K, max_text_len=MAX_LEN)
    g = torch.Generator().manual_seed(0)
    mem = torch.randn(CLIPS, cfg.mem_tokens, cfg.d_model, generator=g).cuda()
    res = dict(k=K, max_len=MAX_LEN, clips=CLIPS, cameras=CAMERAS)
    res["plain_ms"] = p50_ms(lambda: m.beam_search(mem, MAX_LEN, K))
    for n in (1, 3):
        res[f"eos_n{n}_ms"] = p50_ms(lambda: m.beam_search(mem, MAX_LEN, K, eos=True, num_keep_best=n))
        st = {}
        m.beam_search_host(mem, MAX_LEN, K, eos=True, num_keep_best=n, stats=st)
        done = st["done_step"]
        res[f"eos_n{n}_steps_after_all_done"] = 0 if any(d is None for d in done) else MAX_LEN - 1 - max(done)
    cams = torch.randn(CAMERAS, cfg.mem_tokens, cfg.d_model, generator=g).cuda()
    for eos in (False, True):
        pool = m.stream_pool(CAMERAS, hop=10 ** 6, max_len=MAX_LEN, beams=K, eos=eos)
        for s in range(CAMERAS):
            pool.push(cams[s], [s] * cfg.mem_tokens)
        tag = "eos" if eos else "plain"
        res[f"pool_{tag}_ms"] = p50_ms(lambda: pool.caption(list(range(CAMERAS))))
        res[f"one_by_one_{tag}_ms"] = p50_ms(lambda: [pool.caption([s]) for s in range(CAMERAS)])
    print(json.dumps(res))


if __name__ == "__main__":
    main()
