#!/usr/bin/env python
"""Headline benchmark: captions/s (+ p50 step latency) of the GIT caption hot path on MI355X.

Workload (BASELINE.json configs[2], the configuration the metric is quoted on): per GPU a batch of
16 synthetic 6-frame 224x224 clips, GIT-base (ViT-B/16 encoder + 6-layer decoder), bf16 MFMA GEMMs,
20-token greedy decode with EOS disabled so every caption costs the same work.  One "step" = one
pass of the whole path (frames resident in HBM -> caption ids) over that batch.  With N > 1 GPUs
the clips shard embarrassingly (one process per GPU, full weight replica) and the only collective
is an RCCL all_gather of the caption ids (int64 [16, 21] per rank) at the end of every step.

    python bench.py --gpus 1 --steps 20 --warmup 3
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
        --master-port P bench.py --gpus N --steps K --warmup W

A plain run sets up, runs the W warm-up steps and the K timed steps on the timed path, writes the caption ids of
the last timed step if --dump-outputs DIR is given, and prints the JSON result line.  --full adds everything else
the benchmark reports: the pipelined == serial screen, the latency frontier, the serial point, the roofline and
per-kernel breakdown, the other BASELINE configurations, host-fed inputs and the CPU baseline.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "real-time-video-captioning_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np      # noqa: E402
import torch            # noqa: E402

CLIPS_PER_GPU, FRAMES, TOKENS = 16, 6, 20
GFLOP_PER_CAPTION = 341.5          # SURVEY.md par. 8(d): GIT-base F=6 T=20, KV-cached, encoder once
MFMA_PEAK_TFLOPS = 2500.0          # dense bf16 (MI355X_MICROARCH.md)
HBM_PEAK_GBS = 8000.0


def library_source_sha() -> str:
    """Fingerprint of the kernel sources the library was built from (csrc/*.hip, *.h): profiles/ records the same
    fingerprint next to the PMC-derived traffic, so a `roofline.traffic` measured on older kernels is visible."""
    import hashlib
    d = os.path.join(ROOT, "real-time-video-captioning_amd", "csrc")
    hsh = hashlib.sha1()
    for name in sorted(os.listdir(d)):
        if name.endswith((".hip", ".h")):
            hsh.update(name.encode())
            with open(os.path.join(d, name), "rb") as f:
                hsh.update(f.read())
    return hsh.hexdigest()[:12]


def decode_phase_bytes(cfg, clips: int, frames: int, tokens: int) -> float:
    """SURVEY.md par. 8(d): algorithmic HBM bytes of the token loop (bf16): every step reads the decoder + head weights
    once and, per clip, the image + text K/V of all layers."""
    D, V, Ld = cfg.dec_width, cfg.vocab_size, cfg.dec_layers
    weights = (Ld * (4 * D * D + 2 * D * cfg.dec_ffn) + D * V) * 2.0
    s_img = frames * cfg.tokens_per_frame
    kv = sum(clips * Ld * 2 * (s_img + t + 1) * D * 2.0 for t in range(tokens))
    return tokens * weights + kv


def usable_cores() -> int:
    """Every core this process may really use: its affinity mask, capped by the cgroup CPU quota when there is one (a
    1-GPU box gives the job a share of the host; threads beyond the quota only time-slice against each other)."""
    try:
        n = len(os.sched_getaffinity(0))
    except AttributeError:
        n = os.cpu_count() or 1
    for path in ("/sys/fs/cgroup/cpu.max", "/sys/fs/cgroup/cpu/cpu.cfs_quota_us"):
        try:
            with open(path) as f:
                parts = f.read().split()
            if path.endswith("cpu.max"):
                if parts[0] != "max":
                    n = min(n, max(1, int(float(parts[0]) / float(parts[1]) + 0.5)))
            else:
                q = int(parts[0])
                if q > 0:
                    with open("/sys/fs/cgroup/cpu/cpu.cfs_period_us") as g:
                        n = min(n, max(1, int(q / int(g.read().split()[0]) + 0.5)))
            break
        except (OSError, ValueError, IndexError):
            continue
    return max(1, n)


def cpu_baseline(cfg, weights, runs: int = 20, warmups: int = 3):
    """oracle/git_oracle.py (fp32, encoder once + exact KV cache, batch 1) timed on the host cores: the CPU restatement
    of the same path, a bounded sample of the same workload, per SURVEY.md par. 8(d) / BASELINE.md par. 3: 3 warm-ups,
    then >= 20 timed captions; the 6-frame clip the metric is quoted on (`value`) and BASELINE configs[0]'s own shape
    (one frame, 20 greedy tokens: src/inference.py:51) beside it."""
    from gitcap.config import git_base
    from oracle.git_oracle import GitOracle, make_frames
    def sample(orc, frames):
        with torch.no_grad():
            for _ in range(warmups):
                orc.greedy_decode(frames, TOKENS, stop="never")
            times = []
            for i in range(runs):
                t0 = time.perf_counter()
                orc.greedy_decode(frames, TOKENS, stop="never")
                times.append(time.perf_counter() - t0)
                if i % 5 == 4:
                    print(f"[bench] cpu_baseline {i + 1}/{runs} captions, {times[-1] * 1e3:.0f} ms each", file=sys.stderr, flush=True)
        return float(np.median(times)), len(times)

    orc = GitOracle(cfg, weights)
    frames = make_frames(1, FRAMES, cfg.image_size, seed=1234)
    # all the cores this process may use (affinity mask, cgroup quota); where that is more than 16, 16 threads are tried
    # too and the faster setting is kept (a mask wider than the job's real share only oversubscribes) -- both are stated
    cores_all = usable_cores()
    tried = {}
    for c in sorted({cores_all, min(16, cores_all)}, reverse=True):
        torch.set_num_threads(c)
        with torch.no_grad():
            orc.greedy_decode(frames, TOKENS, stop="never")
            t0 = time.perf_counter()
            orc.greedy_decode(frames, TOKENS, stop="never")
            tried[c] = time.perf_counter() - t0
        print(f"[bench] cpu_baseline probe: {c} threads {tried[c] * 1e3:.0f} ms per caption", file=sys.stderr, flush=True)
    cores = min(tried, key=tried.get)
    torch.set_num_threads(cores)
    runs = max(5, min(runs, int(40.0 / max(tried[cores], 1e-3))))      # keep the default bench run within minutes
    med, n = sample(orc, frames)
    # the reference as written (SURVEY.md par. 8d): no KV cache, the whole [image; text] sequence is recomputed
    # for every token (model.py:412-418 under the search loop of :518-519), one clip per call (:765)
    with torch.no_grad():
        t0 = time.perf_counter()
        orc.greedy_decode(frames, TOKENS, stop="never", use_cache=False)
        as_written = time.perf_counter() - t0
    # BASELINE configs[0]: one 224x224 frame, GIT-base (no temporal embedding), 20 greedy tokens
    cfg1 = git_base(0)
    from gitcap.weights import synthetic_weights
    orc1 = GitOracle(cfg1, synthetic_weights(cfg1, seed=0))
    med1, n1 = sample(orc1, make_frames(1, 1, cfg1.image_size, seed=1234))
    return {"value": round(1.0 / med, 4), "unit": "captions/s", "cores": cores, "kind": "port",
            "cores_usable": cores_all, "thread_probe_ms": {str(k): round(v * 1e3, 1) for k, v in tried.items()},
            "as_written": {"value": round(1.0 / as_written, 4), "unit": "captions/s",
                           "sample": "1 caption, same oracle with use_cache=False (full recompute per token)"},
            "single_frame": {"value": round(1.0 / med1, 4), "unit": "captions/s", "p50_latency_ms": round(med1 * 1e3, 1),
                             "sample": f"BASELINE configs[0]: {n1} captions (1 frame x {TOKENS} tokens, batch 1, fp32, KV-cached "
                                       f"oracle) after {warmups} warm-ups"},
            "sample": f"{n} captions (1 clip x {FRAMES} frames x {TOKENS} tokens each, batch 1, fp32, "
                      f"KV-cached oracle) after {warmups} warm-ups; median {med * 1e3:.0f} ms/caption",
            "p50_latency_ms": round(med * 1e3, 1)}


def host_fed(model, cfg, dev, note, steps, inflight, resident_value):
    """The headline workload (configs[2]) with the frames starting in HOST memory, as the reference's callers hold them
    (src/real_time_inference.py:39-58: OpenCV frames; src/inference.py:27, :45-51: a DataLoader batch, pin_memory=True): every
    batch crosses PCIe inside the timed region -- through the pinned staging ring and the copy stream of gitcap/model.py
    (_StagingRing), under the compute of the batches before it.  Never the headline `value` (inputs resident in HBM)."""
    g = torch.Generator(device="cpu").manual_seed(4321)
    NIN = 4
    S = cfg.image_size
    u8 = [torch.randint(0, 256, (CLIPS_PER_GPU, FRAMES, S, S, 3), dtype=torch.uint8, generator=g) for _ in range(NIN)]
    f32 = [torch.randn(CLIPS_PER_GPU, FRAMES, 3, S, S, generator=g) for _ in range(NIN)]
    cases = {
        "pinned_uint8_hwc_bgr_224": ([x.pin_memory() for x in u8], "uint8 HWC BGR 224x224 camera frames, page-locked; the transform of "
                                     "dataloader.py:18-32 runs on the device fused with the patch gather (14.5 MB per batch over PCIe)"),
        "pageable_uint8_hwc_bgr_224": (u8, "the same frames in pageable memory (one parallel copy into the pinned ring first)"),
        "pinned_fp32_nchw": ([x.pin_memory() for x in f32], "transformed fp32 NCHW frames, page-locked: what DataLoader(pin_memory=True) "
                             "of src/inference.py:27 yields (57.8 MB per batch over PCIe)"),
        "pageable_fp32_nchw": (f32, "transformed fp32 NCHW frames in pageable memory (src/utils/dataloader.py:60-82 without pinning)"),
    }
    out = {"workload": "BASELINE configs[2] (16 x 6-frame clips, GIT-base, 20 greedy tokens), frames start in host memory; "
                       f"{inflight} batches in flight, {steps} batches per region, median of 3 regions",
           "resident_captions_per_s": round(resident_value, 1)}
    for name, (ins, what) in cases.items():
        want = [model.greedy_decode(x.to(dev), max_len=TOKENS, stop="never").clone() for x in ins]

        def region(check=False):
            ev_sub = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
            ev_done = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
            ok, pend = True, []
            torch.cuda.synchronize(dev)
            t0 = time.perf_counter()
            for i in range(steps):
                ev_sub[i].record()
                pend.append((i, model.greedy_decode_async(ins[i % NIN], max_len=TOKENS, stop="never")))
                if len(pend) == inflight:
                    j, fut = pend.pop(0)
                    r = fut.result()                      # CPU in -> CPU out: the ids come back to the host as well
                    ev_done[j].record()
                    ok = ok and (not check or bool(torch.equal(r, want[j % NIN].cpu())))
            for j, fut in pend:
                r = fut.result()
                ev_done[j].record()
                ok = ok and (not check or bool(torch.equal(r, want[j % NIN].cpu())))
            torch.cuda.synchronize(dev)
            el = time.perf_counter() - t0
            lat = sorted(ev_sub[i].elapsed_time(ev_done[i]) for i in range(steps))
            return el, lat[len(lat) // 2], ok
        same = region(check=True)[2]
        rs = sorted(region()[:2] for _ in range(3))
        el, p50 = rs[1]
        v = CLIPS_PER_GPU * steps / el
        out[name] = {"what": what, "captions_per_s": round(v, 1), "ms_per_batch": round(el / steps * 1e3, 3), "p50_latency_ms": round(p50, 3),
                     "fraction_of_resident": round(v / resident_value, 4), "ids_equal_resident_path": same}
        note(f"host_fed: {name} {v:.0f} captions/s")
    return out


def other_configs(dev, note):
    """The other BASELINE.json configurations and the reference's one real caller, under the same clock as the headline
    (outside its timed region; parity-test cases otherwise): configs[1] (32 single frames, GIT-base), configs[4] (GIT-large,
    10-frame clips, beam 4, 15 steps, src/models/model.py:702-708; B = 4 clips, e4m3 and bf16 weight storage) and the webcam
    shape of src/real_time_inference.py:56-58 (one 6-frame clip, CPU tensor in, 25 tokens, CPU ids out)."""
    from gitcap.config import git_base, git_large
    from gitcap.model import GitCaptioner
    from gitcap.weights import quantize_weights_fp8, synthetic_weights

    def med_ms(fn, n=7, warm=2):
        for _ in range(warm):
            fn()
        torch.cuda.synchronize(dev)
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize(dev)
            ts.append((time.perf_counter() - t0) * 1e3)
        return sorted(ts)[len(ts) // 2]

    out = {}
    # ---- configs[1]: batch = 32 single-frame image captioning, GIT-base, 20 greedy tokens ----
    cfg = git_base(0)
    w = synthetic_weights(cfg, seed=0)
    m = GitCaptioner(cfg, w, device=dev, max_batch=32, max_frames=1, max_text_len=TOKENS, stop="never")
    g = torch.Generator(device="cpu").manual_seed(99)
    ins = [torch.randn(32, 1, 3, cfg.image_size, cfg.image_size, generator=g).to(dev) for _ in range(2)]
    k = [0]

    def one():
        k[0] += 1
        return m.greedy_decode(ins[k[0] % 2], max_len=TOKENS, stop="never")
    ser = med_ms(one)

    def pipe(n):
        pend = []
        for i in range(n):
            pend.append(m.greedy_decode_async(ins[i % 2], max_len=TOKENS, stop="never"))
            if len(pend) == 4:
                pend.pop(0).result()
        while pend:
            pend.pop(0).result()
    pipe(4)
    torch.cuda.synchronize(dev)
    t0 = time.perf_counter()
    pipe(16)
    torch.cuda.synchronize(dev)
    pp = (time.perf_counter() - t0) / 16 * 1e3
    t1 = med_ms(lambda: m.greedy_decode(ins[0], max_len=1, stop="never"), n=5)
    loop = (ser - t1) * TOKENS / (TOKENS - 1)
    db = decode_phase_bytes(cfg, 32, 1, TOKENS)
    out["configs[1]"] = {"workload": "32 single 224x224 frames, GIT-base, 20 greedy tokens, EOS disabled",
                         "serial_ms_per_batch": round(ser, 3), "serial_captions_per_s": round(32e3 / ser, 1),
                         "pipelined_ms_per_batch": round(pp, 3), "pipelined_captions_per_s": round(32e3 / pp, 1),
                         "gflop_per_caption": 55.6, "pipelined_mfma_frac": round(32e3 / pp * 55.6 / 1e3 / MFMA_PEAK_TFLOPS, 4),
                         "decode_phase_ms": round(loop, 3), "decode_phase_hbm_frac": round(db / (loop * 1e-3) / 1e9 / HBM_PEAK_GBS, 4)}
    del m
    note("other_configs: configs[1] done")
    # ---- configs[2] with the opt-in e4m3 V cache of the token loop (kv_cache="v_e4m3"; the headline stays bf16) ----
    cfg = git_base(FRAMES)
    w6 = synthetic_weights(cfg, seed=0)
    ins6 = [torch.randn(CLIPS_PER_GPU, FRAMES, 3, cfg.image_size, cfg.image_size, generator=g).to(dev) for _ in range(2)]
    rec = {}
    for mode in ("bf16", "v_e4m3"):
        m = GitCaptioner(cfg, w6, device=dev, max_batch=CLIPS_PER_GPU, max_frames=FRAMES, max_text_len=TOKENS, stop="never", kv_cache=mode)
        kk = [0]

        def one6():
            kk[0] += 1
            return m.greedy_decode(ins6[kk[0] % 2], max_len=TOKENS, stop="never")
        ser = med_ms(one6)
        t1 = med_ms(lambda: m.greedy_decode(ins6[0], max_len=1, stop="never"), n=5)
        loop = (ser - t1) * TOKENS / (TOKENS - 1)

        def pipe6(n):
            pend = []
            for i in range(n):
                pend.append(m.greedy_decode_async(ins6[i % 2], max_len=TOKENS, stop="never"))
                if len(pend) == 3:
                    pend.pop(0).result()
            while pend:
                pend.pop(0).result()
        pipe6(4)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        pipe6(18)
        torch.cuda.synchronize(dev)
        pp = (time.perf_counter() - t0) / 18 * 1e3
        rec[mode] = {"serial_ms_per_batch": round(ser, 3), "decode_phase_ms": round(loop, 3), "image_pass_ms": round(t1 - loop / TOKENS, 3),
                     "pipelined_ms_per_batch": round(pp, 3), "pipelined_captions_per_s": round(CLIPS_PER_GPU * 1e3 / pp, 1),
                     "workspace_mbytes": round(m.workspace_bytes() / 1e6, 1)}
        del m
    out["kv_cache_v_e4m3"] = {"workload": "BASELINE configs[2] (16 x 6-frame clips, GIT-base, 20 greedy tokens) with the image prefix's V rows as "
                              "e4m3 codes for the token loop (opt-in; results differ by the rounding of V), beside the default on the same box", **rec}
    note("other_configs: kv_cache v_e4m3 done")
    # ---- the webcam shape: one clip, CPU in / CPU out, 25 tokens (real_time_inference.py:56-58) ----
    cfg = git_base(FRAMES)
    m = GitCaptioner(cfg, synthetic_weights(cfg, seed=0), device=dev, max_batch=1, max_frames=FRAMES, max_text_len=25, stop="never")
    clip = torch.randn(1, FRAMES, 3, cfg.image_size, cfg.image_size, generator=g)
    cpu_io = med_ms(lambda: m.greedy_decode(clip, max_len=25, stop="never"), n=9)
    clip_d = clip.to(dev)
    dev20 = med_ms(lambda: m.greedy_decode(clip_d, max_len=TOKENS, stop="never"), n=9)
    # the same caller before its transform: six 480 x 640 uint8 BGR camera frames (real_time_inference.py:39), pageable host memory,
    # transform fused into the patch gather on the device
    cam = torch.randint(0, 256, (1, FRAMES, 480, 640, 3), dtype=torch.uint8, generator=g)
    cam_io = med_ms(lambda: m.greedy_decode(cam, max_len=25, stop="never"), n=9)
    out["one_clip"] = {"workload": "1 clip x 6 frames, GIT-base; the reference's caller (src/real_time_inference.py:56-58)",
                       "cpu_in_cpu_out_25_tokens_ms": round(cpu_io, 3), "device_resident_20_tokens_ms": round(dev20, 3),
                       "camera_480x640_uint8_cpu_in_cpu_out_25_tokens_ms": round(cam_io, 3),
                       "camera_captions_per_s": round(1e3 / cam_io, 1)}
    del m
    note("other_configs: one clip done")
    # ---- configs[4]: GIT-large, 10-frame clips, beam 4, 15 steps, device-resident search; B = 4 / 8 / 16 clips per batch,
    # one batch at a time (gitcap_beam_search) and three batches in flight (gitcap_beam_search_submit / _wait) ----
    cfg = git_large(10)
    beams, steps = 4, 15
    wq = quantize_weights_fp8(synthetic_weights(cfg, seed=0))
    fr16 = [torch.randn(16, 10, 3, cfg.image_size, cfg.image_size, generator=g).to(dev) for _ in range(2)]
    D, V, Ld, S = cfg.dec_width, cfg.vocab_size, cfg.dec_layers, 10 * cfg.tokens_per_frame
    c4 = {"workload": "GIT-large (ViT-L/14), B clips x 10 frames, beam 4, 15 steps, e4m3-valued weights, device-resident search; "
                      "top-level fields of a storage mode: B = 4", "gflop_per_caption": 1975.0}
    for storage in ("fp8_e4m3", "bf16", "fp8_e4m3+fp8_ffn"):         # the last: FC1 / FC2 of the image rows on fp8 MFMA (opt-in compute)
        m = GitCaptioner(cfg, wq, device=dev, max_batch=16, max_frames=10, max_text_len=20, max_beams=beams,
                         weight_dtype=storage.split("+")[0], compute="fp8_ffn" if storage.endswith("fp8_ffn") else "bf16")
        wbytes = (Ld * (4 * D * D + 2 * D * cfg.dec_ffn) + D * V) * (1.0 if storage.startswith("fp8_e4m3") else 2.0)
        rec = {}
        for B in ((4,) if storage == "bf16" else (4, 8, 16)):
            ins4 = [x[:B] for x in fr16]
            want = m.infer(ins4[0], beam_size=beams, max_steps=steps)["predictions"].clone()
            dt = med_ms(lambda: m.infer(ins4[0], beam_size=beams, max_steps=steps), n=5)
            di = med_ms(lambda: m.forward_image_enc(ins4[0]), n=5)
            kv = sum(B * beams * Ld * 2 * (S + t + 1) * D * 2.0 for t in range(steps - 1))
            lp = dt - di

            def pipe4(n, check=False):
                pend, ok = [], True
                for i in range(n):
                    pend.append((i % 2, m.infer_async(ins4[i % 2], beam_size=beams, max_steps=steps)))
                    if len(pend) == 3:
                        k, f = pend.pop(0)
                        r = f.result()
                        ok = ok and (k != 0 or not check or bool(torch.equal(r["predictions"], want)))
                while pend:
                    k, f = pend.pop(0)
                    r = f.result()
                    ok = ok and (k != 0 or not check or bool(torch.equal(r["predictions"], want)))
                return ok
            same = pipe4(4, check=True)
            torch.cuda.synchronize(dev)
            nb = 12 if B <= 8 else 8
            t0 = time.perf_counter()
            pipe4(nb)
            torch.cuda.synchronize(dev)
            pp = (time.perf_counter() - t0) / nb * 1e3
            r = {"ms_per_batch": round(dt, 3), "captions_per_s": round(B * 1e3 / dt, 1),
                 "mfma_frac": round(B * 1e3 / dt * 1975.0 / 1e3 / MFMA_PEAK_TFLOPS, 4), "image_pass_ms": round(di, 3),
                 "search_loop_ms": round(lp, 3), "search_loop_hbm_frac": round(((steps - 1) * wbytes + kv) / (lp * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                 "pipelined_ms_per_batch": round(pp, 3), "pipelined_captions_per_s": round(B * 1e3 / pp, 1),
                 "pipelined_mfma_frac": round(B * 1e3 / pp * 1975.0 / 1e3 / MFMA_PEAK_TFLOPS, 4),
                 "pipelined_equals_synchronous": same}
            if B == 4:
                rec.update(r)
                rec["weight_mbytes"] = round(m.weight_bytes() / 1e6, 1)
                rec["workspace_mbytes"] = round(m.workspace_bytes() / 1e6, 1)      # incl. the fragment-major weight copies
            else:
                rec[f"B={B}"] = r
        c4[storage] = rec
        del m
        note(f"other_configs: configs[4] {storage} done")
    out["configs[4]"] = c4
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=None,
                    help="the K-step timed region is repeated; the median repeat is reported (default 1, 5 with --full)")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement and check beside the headline (without it: warm-up + the timed steps only)")
    ap.add_argument("--dump-outputs", metavar="DIR",
                    help="write the caption ids of the last timed step to DIR/caption_ids.npy (float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-other-configs", action="store_true",
                    help="with --full: skip configs[1] / configs[4] / one-clip / host-fed (reported beside the headline)")
    ap.add_argument("--no-profile", action="store_true", help="with --full: skip the HIP-event instrumented pass")
    ap.add_argument("--serial", action="store_true", help="one batch at a time (no cross-batch pipelining)")
    ap.add_argument("--inflight", type=int, default=3, choices=(2, 3, 4),
                    help="submissions in flight when pipelined (3: same throughput as 4, lower latency)")
    ap.add_argument("--coalesce", type=int, default=1, choices=(1, 2, 4),
                    help="dynamic batching: run this many consecutive 16-clip batches as one pass")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.repeats is None:
        args.repeats = 5 if args.full else 1

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if args.gpus != world:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch N>1 with torch.distributed.run (one process per GPU); see module docstring")
    phase = ["start", time.time()]

    def note(msg):
        phase[0], phase[1] = msg, time.time()
        if rank == 0:
            print(f"[bench] {msg}", file=sys.stderr, flush=True)

    def heartbeat():            # a run that stops making progress says where, and ends with a status instead of a silent kill
        while True:
            time.sleep(30)
            stuck = time.time() - phase[1]
            print(f"[bench] rank {rank} alive: {stuck:.0f} s since '{phase[0]}'", file=sys.stderr, flush=True)
            if stuck > 600:
                print(f"[bench] rank {rank}: no progress for 10 minutes after '{phase[0]}', giving up", file=sys.stderr, flush=True)
                os._exit(4)
    import threading
    threading.Thread(target=heartbeat, daemon=True).start()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    dist = None
    use_dist = world > 1 or os.environ.get("BENCH_FORCE_DIST") == "1"   # the latter: 1-rank rehearsal of the N>1 path
    json_fd = None
    if use_dist:
        import torch.distributed as dist
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        # RCCL prints a version banner to stdout when its communicator is created: keep the process's stdout for the ONE
        # JSON line (everything else written to fd 1 from here on goes to stderr)
        sys.stdout.flush()
        json_fd = os.dup(1)
        os.dup2(2, 1)
        dist.init_process_group("nccl", device_id=dev)   # "nccl" is RCCL on ROCm

    from gitcap.config import git_base
    from gitcap.model import GitCaptioner
    from gitcap.weights import synthetic_weights

    cfg = git_base(FRAMES)
    weights = synthetic_weights(cfg, seed=0)
    model = GitCaptioner(cfg, weights, device=dev, max_batch=CLIPS_PER_GPU * args.coalesce, max_frames=FRAMES,
                         max_text_len=TOKENS, stop="never")
    # rank r holds clips [r*16, (r+1)*16) of the global batch; inputs are resident in HBM.  Four distinct batches are
    # rotated through so that no step re-reads the previous step's frames from a warm cache.
    NIN = 4
    g = torch.Generator(device="cpu").manual_seed(1234 + 16 * rank)
    inputs = [torch.randn(CLIPS_PER_GPU, FRAMES, 3, cfg.image_size, cfg.image_size, generator=g).to(dev) for _ in range(NIN)]
    # N > 1: the per-batch RCCL gather (int64[16,21] per rank) runs asynchronously into a ring of output buffers
    # (gitcap/dist.py: CaptionGatherRing, covered on CPU by tests/test_dist_gloo.py)
    ring = None
    if use_dist:
        from gitcap.dist import CaptionGatherRing
        ring = CaptionGatherRing(world * CLIPS_PER_GPU, TOKENS + 1, dev, nbuf=8)

    def finish(ids, join=False):
        if ring is None:
            return ids
        _, buf = ring.push(ids, join=join)
        return buf

    def step(i):                                           # one batch, start to finish (gather joined: a caller waits for it)
        return finish(model.greedy_decode(inputs[i % NIN], max_len=TOKENS, stop="never"), join=True)

    def fence():
        if ring is not None:
            ring.fence()                                   # every gather issued so far has completed, then barrier
        torch.cuda.synchronize(dev)

    # K steps = K batches.  Default: three batches in flight (one image pass overlaps the token loops of
    # the batches before it, on the library's streams); every batch is submitted AND completed (ids gathered)
    # inside the timed region.  --serial runs one batch at a time.  The region (barrier + synchronize on both sides,
    # max over ranks) is repeated --repeats times and the median repeat is reported.
    last_ids = [None]                                      # what the region's last step returned to its caller

    def timed_region(inflight=None, serial_mode=None, steps=None):
        inflight = args.inflight if inflight is None else inflight
        serial_mode = args.serial if serial_mode is None else serial_mode
        steps = args.steps if steps is None else steps
        ev_sub = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
        ev_done = [torch.cuda.Event(enable_timing=True) for _ in range(steps)]
        out = None
        fence()
        t0 = time.perf_counter()
        if serial_mode:
            for i in range(steps):
                ev_sub[i].record()
                out = step(i)
                ev_done[i].record()
        else:
            pending = []
            for i in range(steps):
                ev_sub[i].record()
                pending.append((i, model.greedy_decode_async(inputs[i % NIN], max_len=TOKENS, stop="never", coalesce=args.coalesce)))
                if len(pending) == inflight * args.coalesce:
                    j, fut = pending.pop(0)
                    out = finish(fut.result())
                    ev_done[j].record()
            for j, fut in pending:
                out = finish(fut.result())
                ev_done[j].record()
        fence()
        el = time.perf_counter() - t0
        lat = sorted(ev_sub[i].elapsed_time(ev_done[i]) for i in range(steps))   # submit -> ids ready, per batch
        p = lat[len(lat) // 2]
        if use_dist:
            t = torch.tensor([el, p], dtype=torch.float64, device=dev)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            el, p = float(t[0]), float(t[1])
        assert out.shape == (world * CLIPS_PER_GPU, TOKENS + 1)
        last_ids[0] = out
        return el, p

    if args.warmup > 0:                                    # the warm-up runs the timed path, so its first use is not timed
        timed_region(steps=args.warmup)
    note("warm-up done")
    regions = sorted(timed_region() for _ in range(max(1, args.repeats)))
    note("timed regions done")
    elapsed, p50 = regions[len(regions) // 2]
    region_ms = [round(r[0] * 1e3, 3) for r in regions]
    if args.dump_outputs and rank == 0:
        # a view into the library's submission buffers (or the gather ring): copied before anything else runs
        os.makedirs(args.dump_outputs, exist_ok=True)
        np.save(os.path.join(args.dump_outputs, "caption_ids.npy"), last_ids[0].cpu().numpy().astype(np.float64))

    # ---- correctness screen of the path just timed (outside the timed region): clips are independent (model.py:765), so
    # the ids of every rotating input must be BITWISE the same pipelined (the library's streams, --inflight in flight,
    # --coalesce) as one batch at a time on the caller's stream ----
    pipelined_equals_serial = None
    if args.full:
        fence()
        want = [model.greedy_decode(x, max_len=TOKENS, stop="never").clone() for x in inputs]
        ok, pend = True, []
        nscreen = 3 * NIN + (1 if args.coalesce > 1 else 0)        # + 1: the last coalesce group stays partly filled (flushed by result())
        for i in range(nscreen):
            pend.append((i % NIN, model.greedy_decode_async(inputs[i % NIN], max_len=TOKENS, stop="never", coalesce=args.coalesce)))
            if len(pend) == args.inflight * args.coalesce:
                k, fut = pend.pop(0)
                ok = ok and bool(torch.equal(fut.result(), want[k]))
        for k, fut in pend:
            ok = ok and bool(torch.equal(fut.result(), want[k]))
        fence()
        pipelined_equals_serial = ok

    note(f"pipelined == serial screen: {pipelined_equals_serial}")
    # ---- the latency / throughput frontier (BASELINE.json metric: "captions/sec + p50 latency"): the same K-step region with
    # one batch at a time, two and three (four) batches in flight; the headline is one of these points ----
    frontier = None
    if args.full and not args.serial:
        frontier = []
        for nf in (1, 2, 3, 4):
            if nf == args.inflight:
                el_f, p_f = elapsed, p50
            else:
                rs = sorted(timed_region(inflight=max(nf, 2), serial_mode=(nf == 1)) for _ in range(3))
                el_f, p_f = rs[1]
            frontier.append({"batches_in_flight": nf * args.coalesce, "captions_per_s": round(world * CLIPS_PER_GPU * args.steps / el_f, 1),
                             "p50_latency_ms": round(p_f, 3), "headline": nf == args.inflight})
        note("latency frontier done")
    # ---- unpipelined reference point: one batch at a time (what a single real-time caller sees) ----
    serial = None
    if args.full and not args.serial:
        ns = min(args.steps, 10)
        es = [torch.cuda.Event(enable_timing=True) for _ in range(ns + 1)]
        fence()
        es[0].record()
        for i in range(ns):
            step(i)
            es[i + 1].record()
        fence()
        sl = sorted(es[i].elapsed_time(es[i + 1]) for i in range(ns))
        serial = {"captions_per_s_per_gpu": round(CLIPS_PER_GPU / (sum(sl) / ns * 1e-3), 1), "p50_latency_ms": round(sl[ns // 2], 3)}

    # ---- decode phase (the 20-step token loop) against the HBM roofline: serial greedy(max_len=T) - greedy(max_len=1),
    # i.e. T-1 token steps, scaled to T steps; algorithmic bytes of SURVEY.md par. 8(d) ----
    def timed_greedy(max_len, n=8):
        ts = []
        for i in range(n + 2):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            model.greedy_decode(inputs[i % NIN], max_len=max_len, stop="never")
            b.record()
            torch.cuda.synchronize(dev)
            ts.append(a.elapsed_time(b))
        ts = sorted(ts[2:])
        return ts[len(ts) // 2]
    decode = None
    if args.full:
        fence()
        t_full, t_one = timed_greedy(TOKENS), timed_greedy(1)
        loop_ms = (t_full - t_one) * TOKENS / (TOKENS - 1)
        dbytes = decode_phase_bytes(cfg, CLIPS_PER_GPU, FRAMES, TOKENS)
        decode = {"bound": "hbm", "what": f"token loop of one {CLIPS_PER_GPU} x {TOKENS} batch, serial", "ms": round(loop_ms, 3),
                  "us_per_token_step": round(loop_ms * 1e3 / TOKENS, 1), "algorithmic_gbytes": round(dbytes / 1e9, 3),
                  "achieved": round(dbytes / (loop_ms * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                  "frac": round(dbytes / (loop_ms * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
                  "image_pass_ms": round(t_one - loop_ms / TOKENS, 3)}

    # ---- per-kernel-class timing: HIP events recorded by the library on its launch stream ----
    roofline, breakdown = None, None
    if args.full and not args.no_profile:
        # The brackets need one batch at a time (synchronous calls); the kernels are those of the pipelined path.
        model.profile(True)
        nprof = min(args.steps, 5)
        for i in range(nprof):
            model.greedy_decode(inputs[i % NIN], max_len=TOKENS, stop="never")
        torch.cuda.synchronize(dev)
        prof = model.profile_read()
        model.profile(False)
        breakdown = {k: {"ms_per_step": round(v["ms"] / nprof, 4), "launches_per_step": v["launches"] // nprof}
                     for k, v in prof.items()}
        # every big-tile GEMM launch: the plain epilogues + the residual GEMMs that also normalise their output rows
        gp, gl = prof["gemm"], prof["gemm_ln"]
        gm = {k: gp[k] + gl[k] for k in ("ms", "launches", "flops")}
        avg_ms = gm["ms"] / max(1, gm["launches"])
        achieved = gm["flops"] / (gm["ms"] * 1e-3) / 1e12 if gm["ms"] > 0 else 0.0
        # HBM-side bytes per launch of this kernel come from separate rocprofv3 --pmc passes (FETCH_SIZE,
        # WRITE_SIZE; gfx950 x2 fetch correction) recorded in profiles/: bench.py cannot profile itself
        # the newest profiles/rNN_pmc_gemm.json; it records the fingerprint of the kernel sources it was measured on
        import glob
        traffic, traffic_src, traffic_sha = None, None, None
        pmcs = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_gemm.json")))
        if pmcs:
            with open(pmcs[-1]) as f:
                pj = json.load(f)
            traffic, traffic_sha = pj.get("traffic_bytes_per_launch"), pj.get("source_sha")
            traffic_src = f"profiles/{os.path.basename(pmcs[-1])} (rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of bench.py --serial)"
        roofline = {"bound": "mfma", "kernel": "gemm256_kernel", "achieved": round(achieved, 1), "peak": MFMA_PEAK_TFLOPS,
                    "unit": "TFLOP/s", "frac": round(achieved / MFMA_PEAK_TFLOPS, 4), "traffic": traffic,
                    "traffic_source": traffic_src, "traffic_source_sha": traffic_sha, "library_source_sha": library_source_sha(),
                    "traffic_stale": (traffic_sha != library_source_sha()) if traffic is not None else None,
                    "launches_per_step": gm["launches"] // nprof, "avg_launch_ms": round(avg_ms, 4),
                    "algorithmic_gflop_per_launch": round(gm["flops"] / max(1, gm["launches"]) / 1e9, 2),
                    # the residual GEMMs normalise their own output rows (EPI_RESID_LN_*): their brackets contain what used
                    # to be separate launches of the layernorm class (37 per step before; what is left is counted here)
                    "layernorm_launches_per_step": prof["rowops"]["launches"] // nprof}
        def part(v):    # both roofs of a launch class: a residual epilogue moves 4-10 bytes per output element
            t = v["flops"] / (v["ms"] * 1e-3) / 1e12 if v["ms"] > 0 else 0.0
            g = v["bytes"] / (v["ms"] * 1e-3) / 1e9 if v["ms"] > 0 else 0.0
            floor_ms = [v["flops"] / (MFMA_PEAK_TFLOPS * 1e12) * 1e3, v["bytes"] / (HBM_PEAK_GBS * 1e9) * 1e3]
            return {"launches_per_step": v["launches"] // nprof, "avg_launch_ms": round(v["ms"] / max(1, v["launches"]), 4),
                    "achieved": round(t, 1), "frac": round(t / MFMA_PEAK_TFLOPS, 4),
                    "algorithmic_gbytes_per_s": round(g, 1), "hbm_frac": round(g / HBM_PEAK_GBS, 4),
                    "binding_roof": "mfma" if floor_ms[0] >= floor_ms[1] else "hbm",
                    "frac_of_binding_roof": round(max(floor_ms) / v["ms"], 4) if v["ms"] > 0 else None}
        roofline["by_epilogue"] = {"plain (bias / GELU / residual)": part(gp), "residual + LayerNorm of the output rows": part(gl)}
        def rate(cls, key, scale):
            v = prof[cls]
            return round(v[key] / (v["ms"] * 1e-3) / scale, 1) if v["ms"] > 0 and v[key] > 0 else None
        # every kernel class against the roof that bounds it (HIP-event brackets: for the ~5 us text-path
        # kernels the brackets include launch gaps, so those rates are lower bounds)
        roofline["classes"] = {
            "attn_full": {"bound": "mfma", "achieved": rate("attn_full", "flops", 1e12), "peak": MFMA_PEAK_TFLOPS, "unit": "TFLOP/s"},
            "layernorm": {"bound": "hbm", "achieved": rate("rowops", "bytes", 1e9), "peak": HBM_PEAK_GBS, "unit": "GB/s"},
            "attn_text": {"bound": "hbm", "achieved": rate("attn_text", "bytes", 1e9), "peak": HBM_PEAK_GBS, "unit": "GB/s"},
            "skinny_gemm": {"bound": "hbm", "achieved": rate("skinny", "bytes", 1e9), "peak": HBM_PEAK_GBS, "unit": "GB/s"},
        }
        for v in roofline["classes"].values():
            v["frac"] = round(v["achieved"] / v["peak"], 4) if v["achieved"] else None
    if decode is not None:
        roofline = roofline or {}
        roofline["decode_phase"] = decode
        # the same figures as scalars (a reader that keeps only the scalar keys of `roofline` still sees both roofs)
        roofline["decode_phase_frac"] = decode["frac"]
        roofline["decode_phase_gbytes_per_s"] = decode["achieved"]
        roofline["decode_phase_ms"] = decode["ms"]
        roofline["image_pass_ms"] = decode["image_pass_ms"]
    if roofline and "by_epilogue" in roofline:
        be = list(roofline["by_epilogue"].values())
        roofline["plain_gemm_mfma_frac"] = be[0]["frac"]
        roofline["gemm_ln_mfma_frac"] = be[1]["frac"]
        roofline["gemm_ln_hbm_frac"] = be[1]["hbm_frac"]
        roofline["attn_full_mfma_frac"] = roofline["classes"]["attn_full"]["frac"]

    others = None
    if rank == 0 and world == 1 and args.full and not args.no_other_configs:
        hf = host_fed(model, cfg, dev, note, args.steps, args.inflight, world * CLIPS_PER_GPU * args.steps / elapsed)
        del model
        others = other_configs(dev, note)
        others["host_fed"] = hf
    note("GPU measurements done")
    cpu = None
    if rank == 0 and world == 1 and args.full and not args.no_cpu_baseline:
        cpu = cpu_baseline(cfg, weights)

    if rank == 0:
        captions = world * CLIPS_PER_GPU * args.steps
        value = captions / elapsed
        line = {
            "metric": "captions/sec", "value": round(value, 2), "unit": "captions/s", "n_gpus": world,
            "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(elapsed / args.steps * 1e3, 3),
            "repeats": len(regions), "region_ms_sorted": region_ms,
            "p50_latency_ms": round(p50, 3), "higher_is_better": True, "scaling": "weak", "vs_baseline": None,
            "dtype": "bf16", "data": "synthetic",
            "config": {"workload": "BASELINE.json configs[2]: batch=16 6-frame 224x224 clips per GPU, GIT-base "
                                   "(ViT-B/16 + 6-layer decoder), 20-token greedy, EOS disabled",
                       "clips_per_gpu": CLIPS_PER_GPU, "frames": FRAMES, "tokens": TOKENS, "global_batch": world * CLIPS_PER_GPU,
                       "parallelism": f"dp{world}", "batches_in_flight": 1 if args.serial else args.inflight * args.coalesce, "coalesce": args.coalesce, "collective": "all_gather(int64[16,21]) per step" if use_dist else "none", "distinct_input_batches": NIN},
            "caption_mfma_frac": round(value / world * GFLOP_PER_CAPTION / 1e3 / MFMA_PEAK_TFLOPS, 4),
            "pipelined_equals_serial": pipelined_equals_serial, "latency_frontier": frontier,
            "serial": serial, "roofline": roofline, "cpu_baseline": cpu, "other_configs": others, "breakdown": breakdown,
        }
        if pipelined_equals_serial is False:
            # the timed path returned different captions than one batch at a time: the number is not a measurement
            line["value"] = None
            line["error"] = "pipelined captions differ from the synchronous call's (bitwise screen failed)"
        if json_fd is not None:
            os.write(json_fd, (json.dumps(line) + "\n").encode())
        else:
            print(json.dumps(line), flush=True)
    if use_dist:
        dist.destroy_process_group()
    if pipelined_equals_serial is False:
        raise SystemExit(3)


if __name__ == "__main__":
    main()
