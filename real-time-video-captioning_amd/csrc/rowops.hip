// HBM-bound row kernels: LayerNorm (one wave per row, 16-byte vector loads), patch gather
// (im2col of NCHW fp32 frames, coalesced 16-B reads along W), text embedding, token selection.
#include "kernels.h"
#include <algorithm>
#include <cmath>
#include "ln_canon.h"
#include "rowln.h"
#include "lp_partials.h"

namespace {

// ---- LayerNorm -------------------------------------------------------------------------------
// One wave per row; lane holds NV float4 at columns 256*i + 4*lane (1 KiB contiguous per wave-instruction), fp32
// throughout.  CANON (D a multiple of 64): the segmented statistics of ln_canon.h -- 16 lanes x 4 columns are one
// 64-column segment, so (i, lane >> 4) names segment 4 i + (lane >> 4) -- bit for bit what the GEMM epilogue that
// normalises its own rows computes.  Otherwise: two-pass (mean, then centred variance) over the wave.
template <int NV, bool CANON>
__global__ __launch_bounds__(256) void layernorm_kernel(LnArgs a) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= a.rows) return;
    const float* xr = a.x + (size_t)row * a.ldx;
    const bool is_cls = a.cls != nullptr && row % a.cls_period == 0;     // wave-uniform
    f32x4 v[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = i * 256 + lane * 4;
        if (c >= a.D) v[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        else if (is_cls) v[i] = *(const f32x4*)(a.cls + c) + *(const f32x4*)(a.cls_pos + c);
        else v[i] = *(const f32x4*)(xr + c);
    }
    float mean, rstd;
    if (CANON) {
        float2 st[NV];
#pragma unroll
        for (int i = 0; i < NV; ++i) st[i] = ln_seg_stats(v[i]);        // segment 4 i + (lane >> 4), in all of its 16 lanes
        auto seg = [&](int sidx) {                                      // segment sidx -> every lane (compile-time index)
            const int src = (sidx & 3) * 16;
            return float2{__shfl(st[sidx >> 2].x, src), __shfl(st[sidx >> 2].y, src)};
        };
        if (a.D == 768) ln_merge<12>(seg, a.eps, mean, rstd);
        else if (a.D == 1024) ln_merge<16>(seg, a.eps, mean, rstd);
        else if (a.D == 128) ln_merge<2>(seg, a.eps, mean, rstd);
        else if (a.D == 64) ln_merge<1>(seg, a.eps, mean, rstd);
        else if (a.D == 256) ln_merge<4>(seg, a.eps, mean, rstd);
        else if (a.D == 512) ln_merge<8>(seg, a.eps, mean, rstd);
        else { mean = 0.f; rstd = 0.f; }                                // launcher never sends other widths here
    } else {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) s += v[i][0] + v[i][1] + v[i][2] + v[i][3];
        mean = wave_sum(s) / (float)a.D;
        float q = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int c = i * 256 + lane * 4;
            if (c < a.D) {
#pragma unroll
                for (int e = 0; e < 4; ++e) { const float d = v[i][e] - mean; q += d * d; }
            }
        }
        rstd = rsqrtf(wave_sum(q) / (float)a.D + a.eps);
    }
    const float* addv = a.add_vec ? a.add_vec + (size_t)((row / a.add_div) % a.add_mod) * a.D : nullptr;
    const bool two = CANON && a.gamma2 != nullptr;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int c = i * 256 + lane * 4;
        if (c < a.D) {
            const f32x4 g = *(const f32x4*)(a.gamma + c);
            const f32x4 b = *(const f32x4*)(a.beta + c);
            f32x4 y;
            if (CANON) {
                y = ln_apply(v[i], mean, rstd, g, b);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) y[e] = (v[i][e] - mean) * rstd * g[e] + b[e];
            }
            if (addv) y += *(const f32x4*)(addv + c);
            if (a.out_f32) *(f32x4*)(a.out_f32 + (size_t)row * a.ld_f32 + c) = y;
            if (a.out_bf16 && !two) {
                uint2 o;
                o.x = pack_bf2(y[0], y[1]);
                o.y = pack_bf2(y[2], y[3]);
                *(uint2*)(a.out_bf16 + (size_t)row * a.ld_bf16 + c) = o;
            }
            v[i] = y;
        }
    }
    if (CANON) {
        if (two) {       // second LayerNorm over the values just produced (what a second launch would read back)
            float2 st[NV];
#pragma unroll
            for (int i = 0; i < NV; ++i) st[i] = ln_seg_stats(v[i]);
            auto seg = [&](int sidx) {
                const int src = (sidx & 3) * 16;
                return float2{__shfl(st[sidx >> 2].x, src), __shfl(st[sidx >> 2].y, src)};
            };
            float mean2, rstd2;
            if (a.D == 768) ln_merge<12>(seg, a.eps2, mean2, rstd2);
            else if (a.D == 1024) ln_merge<16>(seg, a.eps2, mean2, rstd2);
            else if (a.D == 128) ln_merge<2>(seg, a.eps2, mean2, rstd2);
            else if (a.D == 64) ln_merge<1>(seg, a.eps2, mean2, rstd2);
            else if (a.D == 256) ln_merge<4>(seg, a.eps2, mean2, rstd2);
            else ln_merge<8>(seg, a.eps2, mean2, rstd2);
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = i * 256 + lane * 4;
                if (c < a.D && a.out_bf16) {
                    const f32x4 y = ln_apply(v[i], mean2, rstd2, *(const f32x4*)(a.gamma2 + c), *(const f32x4*)(a.beta2 + c));
                    uint2 o;
                    o.x = pack_bf2(y[0], y[1]);
                    o.y = pack_bf2(y[2], y[3]);
                    *(uint2*)(a.out_bf16 + (size_t)row * a.ld_bf16 + c) = o;
                }
            }
        }
    }
}

// ---- im2col ----------------------------------------------------------------------------------
// thread = 4 consecutive px of one (patch row, c, py): one 16-B fp32 read, one 8-B bf16 write.
// p % 4 == 0 fast path; generic path handles p = 14 (ViT-L/14) with 2-element pieces.
template <int VEC>
__global__ __launch_bounds__(256) void im2col_kernel(const float* __restrict__ frames, bf16_t* __restrict__ out,
                                                     int nf, int img, int p, int Kp) {
    const int G = img / p;
    const int kvec = Kp / VEC;                                   // pieces per patch row (incl. zero pad)
    const int64_t total = (int64_t)nf * G * G * kvec;
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int kv = (int)(idx % kvec);
    const int64_t prow = idx / kvec;                             // frame*G*G + gy*G + gx
    const int k = kv * VEC;
    bf16_t* o = out + prow * Kp + k;
    if (k >= 3 * p * p) {
#pragma unroll
        for (int e = 0; e < VEC; ++e) o[e] = 0;
        return;
    }
    const int gx = (int)(prow % G), gy = (int)((prow / G) % G);
    const int64_t frame = prow / (G * G);
    const int c = k / (p * p), rem = k - c * p * p, py = rem / p, px = rem - py * p;
    const float* src = frames + ((frame * 3 + c) * img + (gy * p + py)) * (int64_t)img + gx * p + px;
    if (VEC == 4) {
        const f32x4 v = *(const f32x4*)src;
        uint2 w;
        w.x = pack_bf2(v[0], v[1]);
        w.y = pack_bf2(v[2], v[3]);
        *(uint2*)o = w;
    } else {
        *(unsigned*)o = pack_bf2(src[0], src[1]);
    }
}



__global__ void cast_bf16_kernel(const float* __restrict__ in, bf16_t* __restrict__ out, int64_t n4) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n4) return;
    const f32x4 v = *(const f32x4*)(in + i * 4);
    uint2 w;
    w.x = pack_bf2(v[0], v[1]);
    w.y = pack_bf2(v[2], v[3]);
    *(uint2*)(out + i * 4) = w;
}

// per-layer hidden states -> caller layout [B][entries][S_img + T][D]; one 256-thread block per output row
__global__ __launch_bounds__(256) void gather_hidden_kernel(const float* __restrict__ img, const float* __restrict__ txt,
                                                            float* __restrict__ out, int n_entries, int S_img, int T, int D,
                                                            size_t img_stride, size_t txt_stride) {
    const int S = S_img + T;
    const size_t row = blockIdx.x;                       // ((b * n_entries) + e) * S + s
    const int s = (int)(row % S), e = (int)((row / S) % n_entries), b = (int)(row / ((size_t)S * n_entries));
    const float* src = s < S_img ? img + e * img_stride + ((size_t)b * S_img + s) * D
                                 : txt + e * txt_stride + ((size_t)b * T + (s - S_img)) * D;
    for (int c = threadIdx.x * 4; c < D; c += 1024) *(f32x4*)(out + row * D + c) = *(const f32x4*)(src + c);
}

// ---- frame window (gitcap_window_*) ----------------------------------------------------------
// push: the ln_post rows of B x n new frames ([B][n][rows_per_frame][D], contiguous) -> ring slots (head + j) % F of their
// clip ([B][F][rows_per_frame][D]).  A plain copy, 16 B per lane; blockIdx.y = frame (b, j).
__global__ __launch_bounds__(256) void window_scatter_kernel(const float* __restrict__ src, float* __restrict__ ring, int n, int F,
                                                             int head, int64_t frame4) {
    const int fr = blockIdx.y, b = fr / n, j = fr % n;
    const float* s = src + (size_t)fr * frame4 * 4;
    float* d = ring + ((size_t)b * F + (head + j) % F) * frame4 * 4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < frame4; i += (int64_t)gridDim.x * 256)
        *(f32x4*)(d + i * 4) = *(const f32x4*)(s + i * 4);
}

// caption: row (b, f, tok) of the decoder input = bf16(ring[b][(head + f) % F][tok] + temporal[f]), optionally also the fp32 sum
// (visual features).  One wave per row, lane = 4 consecutive columns, as layernorm_kernel; the add is the one the fused ln_post
// epilogue makes (a lone fp32 add, compiled without contraction) and the rounding its pack_bf2, so the bits are gitcap_encode's.
__global__ __launch_bounds__(256) void window_assemble_kernel(const float* __restrict__ ring, const float* __restrict__ temporal,
                                                              bf16_t* __restrict__ out, float* __restrict__ vis, int rows, int F,
                                                              int head, int N, int D) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int tok = row % N, f = (row / N) % F, b = row / (N * F);
    const float* src = ring + (((size_t)b * F + (head + f) % F) * N + tok) * D;
    const float* t = temporal ? temporal + (size_t)f * D : nullptr;
    for (int c = lane * 4; c < D; c += 256) {
        f32x4 y = *(const f32x4*)(src + c);
        if (t) y += *(const f32x4*)(t + c);
        if (vis) *(f32x4*)(vis + (size_t)row * D + c) = y;
        uint2 o;
        o.x = pack_bf2(y[0], y[1]);
        o.y = pack_bf2(y[2], y[3]);
        *(uint2*)(out + (size_t)row * D + c) = o;
    }
}

// ---- ragged batches (gitcap_attach_frame_counts) ------------------------------------------------
// The tables of a packed batch from its per-clip frame counts (by value: at most 256 clips).  One thread: a few hundred adds.
__global__ __launch_bounds__(64) void ragged_tables_kernel(RaggedCounts rc, int N, int32_t* __restrict__ off, int32_t* __restrict__ len,
                                                           int32_t* __restrict__ pos) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    int frame = 0;
    for (int b = 0; b < rc.B; ++b) {
        const int n = rc.n[b];
        off[b] = frame * N;
        len[b] = n * N;
        for (int f = 0; f < n; ++f) pos[frame + f] = f;
        frame += n;
    }
}

// window_assemble_kernel with the frame's position read from pos[] and the rows read in place: one wave per row, lane = 4
// consecutive columns; a lone fp32 add (no contraction) and pack_bf2, so the bits are the fused ln_post epilogue's.
__global__ __launch_bounds__(256) void ragged_temporal_kernel(const float* __restrict__ ln, const float* __restrict__ temporal,
                                                              const int32_t* __restrict__ pos, bf16_t* __restrict__ out,
                                                              float* __restrict__ vis, int rows, int N, int D) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* src = ln + (size_t)row * D;
    const float* t = temporal + (size_t)pos[row / N] * D;
    for (int c = lane * 4; c < D; c += 256) {
        f32x4 y = *(const f32x4*)(src + c);
        y += *(const f32x4*)(t + c);
        if (vis) *(f32x4*)(vis + (size_t)row * D + c) = y;
        uint2 o;
        o.x = pack_bf2(y[0], y[1]);
        o.y = pack_bf2(y[2], y[3]);
        *(uint2*)(out + (size_t)row * D + c) = o;
    }
}

// e4m3 weight panel -> bf16 staging panel for the big-tile GEMMs (16 values per thread: 16-B read, 32-B write)
__global__ __launch_bounds__(256) void dequant_fp8_kernel(const unsigned char* __restrict__ w8, const float* __restrict__ scale,
                                                          bf16_t* __restrict__ out, int K, int64_t n16) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n16) return;
    const int64_t e = i * 16;
    const float sc = scale[e / K];
    const uint4 q = *(const uint4*)(w8 + e);
    const bf16x8 lo = fp8x8_to_bf16x8(make_uint2(q.x, q.y), sc), hi = fp8x8_to_bf16x8(make_uint2(q.z, q.w), sc);
    const uint4 o4l = __builtin_bit_cast(uint4, lo), o4h = __builtin_bit_cast(uint4, hi);
    const unsigned o[8] = {o4l.x, o4l.y, o4l.z, o4l.w, o4h.x, o4h.y, o4h.z, o4h.w};
    *(uint4*)(out + e) = make_uint4(o[0], o[1], o[2], o[3]);
    *(uint4*)(out + e + 8) = make_uint4(o[4], o[5], o[6], o[7]);
}

__global__ __launch_bounds__(256) void dequant_fp8_batch_kernel(DequantBatch b) {
    const int which = blockIdx.y;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (which >= b.n || i >= b.n16[which]) return;
    const int64_t e = i * 16;
    const float sc = b.scale[which][e / b.K[which]];
    const uint4 q = *(const uint4*)(b.w8[which] + e);
    const bf16x8 lo = fp8x8_to_bf16x8(make_uint2(q.x, q.y), sc), hi = fp8x8_to_bf16x8(make_uint2(q.z, q.w), sc);
    *(uint4*)(b.out[which] + e) = __builtin_bit_cast(uint4, lo);
    *(uint4*)(b.out[which] + e + 8) = __builtin_bit_cast(uint4, hi);
}

// ---- text embedding + LayerNorm: one wave per (row, position) (rowln.h) --------------------------
template <int NV>
__global__ __launch_bounds__(256) void embed_text_kernel(const int64_t* __restrict__ ids, int ld_ids, int rows, int T,
                                                         int t0, const float* __restrict__ word,
                                                         const float* __restrict__ pos, const float* __restrict__ gamma,
                                                         const float* __restrict__ beta, float eps, int D, int vocab,
                                                         float* __restrict__ xf, bf16_t* __restrict__ xb) {
    const int lane = threadIdx.x & 63;
    const int m = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (m >= rows * T) return;
    f32x4 v[NV];
    const float s = row_load_embed<NV>(v, ids, ld_ids, T, t0, word, pos, D, vocab, m, lane);
    row_layernorm<NV>(v, s, lane, D, eps, gamma, beta);
    row_store<NV>(v, lane, D, xf ? xf + (size_t)m * D : nullptr, xb ? xb + (size_t)m * D : nullptr);   // either may be null (row_store)
}

// ---- split-K reduce + bias + residual + LayerNorm (text rows) (rowln.h) ---------------------------------------------
// One workgroup per row, one wave per group of 8 slabs: every wave sums its group (row_slab_tree), wave 0 adds the group
// sums in ascending order, then bias + residual, and normalises the row.  With up to 8 slabs that is one wave, the kernel of
// rounds 1-3; the fused FC1 -> GELU -> FC2 launch of round 4 (ffn_txt.hip) leaves dec_ffn / 64 = 48 slabs, 147 KB per
// row: six waves fetch them side by side.  Same bits as row_load_reduce in one wave (the row prologue of skinny.hip).
template <int NV>
__global__ __launch_bounds__(512) void ln_reduce_kernel(const float* __restrict__ slabs, int nslab,
                                                        const float* __restrict__ bias, const float* __restrict__ resid,
                                                        const float* __restrict__ gamma, const float* __restrict__ beta,
                                                        float eps, int M, int D, float* __restrict__ xf,
                                                        bf16_t* __restrict__ xb) {
    __shared__ __attribute__((aligned(16))) float part[7][NV * 256];           // group sums of waves 1..7
    const int lane = threadIdx.x & 63, g = threadIdx.x >> 6, m = blockIdx.x;
    const int ngroups = (nslab + 7) >> 3;
    // bias, residual row, gamma and beta of the row: requested before the slabs (every wave: a branch around the loads would be
    // waited for where it ends), in flight behind the slab tree and the merge instead of four round trips of wave 0 after them
    f32x4 bv[NV], rv[NV], gv[NV], bev[NV];
    row_load_vec<NV>(bv, bias, D, lane);
    row_load_vec<NV>(rv, resid + (size_t)m * D, D, lane);
    row_load_vec<NV>(gv, gamma, D, lane);
    row_load_vec<NV>(bev, beta, D, lane);
    f32x4 v[NV];
    row_slab_tree<NV>(v, slabs, nslab, g * 8, M, D, m, lane);
    if (ngroups > 1) {
        if (g > 0) {
#pragma unroll
            for (int i = 0; i < NV; ++i) *(f32x4*)(&part[g - 1][i * 256 + lane * 4]) = v[i];
        }
        __syncthreads();
        if (g > 0) return;
        for (int j = 1; j < ngroups; ++j)
#pragma unroll
            for (int i = 0; i < NV; ++i) v[i] += *(const f32x4*)(&part[j - 1][i * 256 + lane * 4]);
    }
    // (0 + t0) + t1 + ... of row_load_reduce: 0 + t0 == t0 exactly
    const float s = row_add_bias_resid_v<NV>(v, bv, rv, D, lane);
    row_layernorm_v<NV>(v, s, lane, D, eps, gv, bev);
    row_store<NV>(v, lane, D, xf + (size_t)m * D, xb + (size_t)m * D);
}

// ---- fragment-major copy of a GEMM weight for the weight-streaming text kernels ------------------------------------------
// src [Npad16][K] (ESZ-byte elements: bf16, or e4m3 codes) -> dst [tile = n / 16][k32 = k / 32][lane][8 elements] with
// lane = n % 16 + 16 * ((k % 32) / 8): the MFMA operand a lane of skinny.hip / txtblock.hip / ffn_txt.hip loads for k-step
// k32 of tile n / 16 is 16 (8) contiguous bytes, a wave instruction reads 1 KiB (512 B) contiguous and a tile's fragments
// are one contiguous run.  Measured (tools/probe/pull_probe.hip): a CU pulls 48 KiB per wave at 47 GB/s in the row-major
// pattern (16 segments of 64 B per instruction) and at 170 GB/s (71 from cold caches) from this layout.
template <typename T>
__global__ __launch_bounds__(256) void pack_frags_kernel(const T* __restrict__ src, T* __restrict__ dst, int K, int64_t total8) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;            // one 8-element fragment piece per thread
    if (i >= total8) return;
    const int lane = (int)(i & 63);
    const int64_t tk = i >> 6;
    const int K32 = K >> 5;
    const int64_t tile = tk / K32;
    const int k32 = (int)(tk - tile * K32);
    const T* sp = src + ((size_t)tile * 16 + (lane & 15)) * K + k32 * 32 + (lane >> 4) * 8;
    T* dp = dst + (size_t)i * 8;
    if (sizeof(T) == 2) *(uint4*)dp = *(const uint4*)sp;
    else *(uint2*)dp = *(const uint2*)sp;
}

// ---- final arg-max over the per-tile partials written by the vocabulary-head kernel ------------
// The arg-max of one row's partials at val / idx + base by a 256-thread workgroup: the largest value, the smallest index among
// equals, 0 for an all-NaN row.  In two parts, both called by argmax_final_kernel and draft_accept_kernel (the one statement of the
// tie rule): argmax_partials_waves, by every thread, leaves each wave's candidate in sv / si (four words of LDS each) behind a
// barrier and thread 0's own in best / bi; argmax_partials_pick, by thread 0 alone, returns the row's.
__device__ __forceinline__ void argmax_partials_waves(const float* __restrict__ val, const int* __restrict__ idx, const size_t base,
                                                      const int ntiles, float* sv, int* si, float& best, int& bi) {
    const int tid = threadIdx.x;
    best = -INFINITY;
    bi = 0x7fffffff;
    // eight partials per thread and round trip (30 522 words = 1908 tiles: one round trip instead of eight); an index past the end
    // re-reads the last tile, which cannot change the result (max value, smallest index among equals: order does not matter)
    for (int i0 = tid; i0 < ntiles; i0 += 256 * 8) {
        float v8[8];
        int j8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = min(i0 + 256 * u, ntiles - 1);
            v8[u] = val[base + i];
            j8[u] = idx[base + i];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u)
            if (v8[u] > best || (v8[u] == best && j8[u] < bi)) { best = v8[u]; bi = j8[u]; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float v2 = __shfl_xor(best, o);
        const int i2 = __shfl_xor(bi, o);
        if (v2 > best || (v2 == best && i2 < bi)) { best = v2; bi = i2; }
    }
    if ((tid & 63) == 0) { sv[tid >> 6] = best; si[tid >> 6] = bi; }
    __syncthreads();
}
__device__ __forceinline__ int argmax_partials_pick(const float* sv, const int* si, float best, int bi, float* vmax = nullptr) {
    for (int w = 1; w < 4; ++w)
        if (sv[w] > best || (sv[w] == best && si[w] < bi)) { best = sv[w]; bi = si[w]; }
    if (bi == 0x7fffffff) bi = 0;
    if (vmax) *vmax = best;
    return bi;
}
// lp_partials (lp_partials.h): the row's log-sum-exp from the head's three partials, in one fixed add order

// The prompt of a forced selection (gitcap_attach_prompt): ids int64 [rows][ld], lengths int32 [rows] (valid tokens, CLS included,
// clamped to [1, max_len] here: max_len <= ld is the host's check, so no read leaves a row), pos = the position the launch writes.
// <false> is empty: the launches without a prompt carry nothing.
template <bool FORCED> struct PromptSel {};
template <> struct PromptSel<true> { const int64_t* ids; const int32_t* lengths; int ld, max_len, pos; };
__device__ __forceinline__ int prompt_len(const int32_t* __restrict__ lengths, const int r, const int max_len) {
    return min(max(lengths[r], 1), max_len);
}

// LP: also lp_out[r * ld_lp] = the log-probability of the token (lp_partials); a form of its own, so that the launches without it
// stay the code they were.  FORCED (again a form of its own): a row whose prompt covers the position written (pr.pos <
// lengths[r]) takes the prompt's token there instead of the arg-max -- into out, and into the next step's embedded row -- does not
// count it in sep_cnt (the stop rule looks at what the model emitted) and writes 0.0f for its log-probability.
// KEEP (a form of its own as well; the tail of a verified draft, gitcap.hip: greedy_draft_loop): a row whose verified part covers
// the position written (kp.pos < kp.len[r], len = valid tokens, CLS included: draft_accept_rows_kernel's) keeps out[r] and
// lp_out[r] as they are -- the accept kernel wrote the loop's own token and log-probability there -- leaves sep_cnt alone (the
// accept kernel counted that position) and embeds the next step's input row from the id already stored.  Every other row is the
// plain kernel.
template <bool KEEP> struct KeepSel {};
template <> struct KeepSel<true> { const int32_t* len; int pos; };
template <int NV, bool LP = false, bool FORCED = false, bool KEEP = false>
__global__ __launch_bounds__(256) void argmax_final_kernel(const float* __restrict__ val, const int* __restrict__ idx,
                                                           int ntiles, int row_stride, int row_off,
                                                           int64_t* __restrict__ out, int ld_out,
                                                           int32_t* __restrict__ sep_cnt, int step, int sep_id, NextEmbed emb,
                                                           const float* __restrict__ psum = nullptr, float* __restrict__ lp_out = nullptr,
                                                           int ld_lp = 0, PromptSel<FORCED> pr = PromptSel<FORCED>{},
                                                           KeepSel<KEEP> kp = KeepSel<KEEP>{}) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ int chosen;
    __shared__ float vmax, ss[4];
    const int r = blockIdx.x, tid = threadIdx.x;
    bool forced = false;                                                   // (thread 0's is the row's; a kept row counts as forced)
    const size_t base = (size_t)(r * row_stride + row_off) * ntiles;
    // gamma / beta of the next step's input row do not depend on the token chosen below: requested now (wave 0 uses them)
    f32x4 gv[NV > 0 ? NV : 1], bv[NV > 0 ? NV : 1];
    if (NV > 0) {
        row_load_vec<(NV > 0 ? NV : 1)>(gv, emb.gamma, emb.D, tid & 63);
        row_load_vec<(NV > 0 ? NV : 1)>(bv, emb.beta, emb.D, tid & 63);
    }
    float best;
    int bi;
    argmax_partials_waves(val, idx, base, ntiles, sv, si, best, bi);
    if (tid == 0) {
        bi = argmax_partials_pick(sv, si, best, bi, LP ? &vmax : nullptr);
        if constexpr (FORCED) {
            forced = pr.pos < prompt_len(pr.lengths, r, pr.max_len);
            if (forced) {
                const int64_t tok = pr.ids[(size_t)r * pr.ld + pr.pos];
                out[(size_t)r * ld_out] = tok;
                chosen = tok < 0 ? -1 : (tok > 0x7fffffff ? 0x7fffffff : (int)tok);   // (the embedding clamps into its table)
            }
        }
        if constexpr (KEEP) {
            forced = kp.pos < kp.len[r];
            if (forced) {
                const int64_t tok = out[(size_t)r * ld_out];
                chosen = tok < 0 ? -1 : (tok > 0x7fffffff ? 0x7fffffff : (int)tok);
            }
        }
        if (!forced) {
            out[(size_t)r * ld_out] = bi;
            if (sep_cnt && bi == sep_id) atomicAdd(&sep_cnt[step], 1);
            chosen = bi;
        }
    }
    if (LP) {
        __syncthreads();
        const float lp = lp_partials(val, psum, base, ntiles, vmax, ss);
        if constexpr (KEEP) {
            if (tid == 0 && !forced) lp_out[(size_t)r * ld_lp] = lp;
        } else {
            if (tid == 0) lp_out[(size_t)r * ld_lp] = forced ? 0.0f : lp;
        }
    }
    if (NV > 0) {       // the next step's input row: embedding of the token just chosen + LayerNorm (one wave)
        __syncthreads();
        if (tid < 64) {
            f32x4 v[NV > 0 ? NV : 1];
            const float s = row_load_embed_tok<(NV > 0 ? NV : 1)>(v, (int64_t)chosen, emb.position, emb.word, emb.pos, emb.D, emb.vocab, tid);
            row_layernorm_v<(NV > 0 ? NV : 1)>(v, s, tid, emb.D, emb.eps, gv, bv);
            row_store<(NV > 0 ? NV : 1)>(v, tid, emb.D, emb.xf + (size_t)r * emb.D, emb.xb + (size_t)r * emb.D);
        }
    }
}

// ---- draft verification of the student's greedy loop (student.hip: greedy_draft_core) -------------------------------------
// The verify pass has left the arg-max partials of all rows x n positions (row m = r * n + j: what the model emits after the
// draft's tokens 0..j of caption r).  One workgroup per (r, j) reduces its row with argmax_partials_waves / _pick -- the tie rule of the
// token loop -- and hands the token to the last workgroup to arrive (txtblock.hip's hand-off: agent-scope store, vmcnt drain,
// barrier, one ticket, agent-scope loads; the ticket word is zero between launches).  That workgroup's first wave, lane j =
// position j, then does the bookkeeping of the covered steps:
//   a_r = leading positions of row r whose token equals the draft's next token ids[r][j + 1] (an id outside the vocabulary was
//         staged as -1 and equals no token); a = min over the rows -- the loop advances all rows in lockstep;
//   covered = a + 1 steps when a < n (the token at position a is the model's own: the corrected token costs no step), else n;
//   ids[r][1 .. covered] = the model's tokens (columns 1..a are the accepted draft tokens, the same values);
//   sep_cnt[t] = rows whose token at step t < covered is SEP, counted from the model's tokens as the token loop counts them;
//   host[0] = a, host[1] = 1 when all rows emitted SEP in one of the covered steps (page-locked host words).
// LP: every workgroup also computes its position's log-probability (lp_partials) and hands its bits over beside the token
// (lp_tok: int[B * n]); the bookkeeping wave writes those of the covered positions to lp_out[r * ld_lp + j] and nothing behind them.
template <bool LP>
__global__ __launch_bounds__(256) void draft_accept_kernel(const float* __restrict__ val, const int* __restrict__ idx, int ntiles, int B,
                                                           int n, int64_t* ids, int ld, int* tok, unsigned* ticket,
                                                           int32_t* __restrict__ sep_cnt, int sep_id, int32_t* host,
                                                           const float* __restrict__ psum, int* lp_tok, float* lp_out, int ld_lp) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ int last_flag;
    __shared__ float vmax, ss[4];
    const int m = blockIdx.x, tid = threadIdx.x;
    float best;
    int bi;
    argmax_partials_waves(val, idx, (size_t)m * ntiles, ntiles, sv, si, best, bi);
    if (tid == 0)
        __hip_atomic_store(tok + m, argmax_partials_pick(sv, si, best, bi, LP ? &vmax : nullptr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (LP) {
        __syncthreads();
        const float lp = lp_partials(val, psum, (size_t)m * ntiles, ntiles, vmax, ss);
        if (tid == 0) __hip_atomic_store(lp_tok + m, __float_as_int(lp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const unsigned old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = old == gridDim.x - 1;
        if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
        last_flag = last;
    }
    __syncthreads();
    if (!last_flag || tid >= 64) return;
    const int j = tid;                                                      // n <= 63: one lane per position
    int a = n;
    for (int r = 0; r < B; ++r) {
        const int t = j < n ? __hip_atomic_load(tok + r * n + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : -1;
        const bool match = j < n && (int64_t)t == ids[(size_t)r * ld + j + 1];
        const unsigned long long miss = __ballot(!match);                   // lanes >= n miss: never zero
        a = min(a, (int)__ffsll((long long)miss) - 1);
    }
    const int covered = a < n ? a + 1 : n;
    int seps = 0;
    for (int r = 0; r < B; ++r) {
        if (j < covered) {
            const int t = __hip_atomic_load(tok + r * n + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            ids[(size_t)r * ld + j + 1] = t;
            seps += t == sep_id;
            if (LP)
                lp_out[(size_t)r * ld_lp + j] = __int_as_float(__hip_atomic_load(lp_tok + r * n + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
        }
    }
    if (j < covered) sep_cnt[j] = seps;
    const bool fired = __ballot(j < covered && seps == B) != 0ull;
    if (j == 0) { host[0] = a; host[1] = fired ? 1 : 0; }
}

// ---- draft verification of the teacher's greedy loop, accepted row by row (gitcap.hip: greedy_draft_loop) -------------------
// column 0 = CLS whatever the draft holds, columns 1..n the draft's tokens, an id outside [0, vocab) as -1: the embedding clamps it
// into its table, it equals no arg-max, so it can only be rejected
__global__ void draft_stage_kernel(const int64_t* __restrict__ draft, int ld_draft, int n, int rows, int vocab, int64_t cls,
                                   int64_t* __restrict__ ids, int ld) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * (n + 1)) return;
    const int r = i / (n + 1), c = i % (n + 1);
    const int64_t d = draft[(size_t)r * ld_draft + c];
    ids[(size_t)r * ld + c] = c == 0 ? cls : (d >= 0 && d < vocab ? d : -1);
}
// draft_accept_kernel's pass (row m = r * n + j, one workgroup each, the same reduction, the same hand-off), but every caption
// keeps what IT accepted: a batch's rows do not wait for its worst one.  Two tickets: the last workgroup of caption r to arrive
// (ticket[1 + r]) does that caption's bookkeeping with its first wave, lane j = position j --
//   a_r = leading positions whose token equals the draft's next token ids[r][j + 1] (-1 equals no token);
//   covered_r = min(a_r + 1, n): the first differing position already holds the loop's own token;
//   ids[r][1 .. covered_r] = the model's tokens, len[r] = 1 + covered_r (valid tokens, CLS included: what KeepSel reads);
//   sep_cnt[j] += 1 for every covered j whose token is SEP (integer atomics: order independent);
//   LP: lp_out[r * ld_lp + j] for j < covered_r; host_rows[r] = a_r (nullable, page-locked);
//   row_res[2 r], [2 r + 1] = covered_r, a_r for the last caption
// -- and the last caption to finish (ticket[0]) publishes host[0..3] = min covered, max covered, sum of a_r, fired (some step
// j < min covered at which sep_cnt[j] == B: every row emitted SEP there).  Nothing behind a caption's covered part is written.
// All ticket words are zero between launches.
template <bool LP>
__global__ __launch_bounds__(256) void draft_accept_rows_kernel(const float* __restrict__ val, const int* __restrict__ idx, int ntiles,
                                                                int B, int n, int64_t* ids, int ld, int32_t* len, int* tok,
                                                                int* row_res, unsigned* ticket, int32_t* sep_cnt, int sep_id,
                                                                int32_t* host, int32_t* host_rows, const float* __restrict__ psum,
                                                                int* lp_tok, float* lp_out, int ld_lp) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ int last_flag;
    __shared__ float vmax, ss[4];
    const int m = blockIdx.x, tid = threadIdx.x;
    const int r = m / n;
    float best;
    int bi;
    argmax_partials_waves(val, idx, (size_t)m * ntiles, ntiles, sv, si, best, bi);
    if (tid == 0)
        __hip_atomic_store(tok + m, argmax_partials_pick(sv, si, best, bi, LP ? &vmax : nullptr), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (LP) {
        __syncthreads();
        const float lp = lp_partials(val, psum, (size_t)m * ntiles, ntiles, vmax, ss);
        if (tid == 0) __hip_atomic_store(lp_tok + m, __float_as_int(lp), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if (tid == 0) {
        const unsigned old = __hip_atomic_fetch_add(ticket + 1 + r, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        const int last = old == (unsigned)n - 1;
        if (last) __hip_atomic_store(ticket + 1 + r, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);   // ready for the next launch
        last_flag = last;
    }
    __syncthreads();
    if (!last_flag || tid >= 64) return;
    // the caption's bookkeeping: one wave, no barrier from here on
    const int j = tid;                                                      // n <= 63: one lane per position
    const int t = j < n ? __hip_atomic_load(tok + r * n + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : -1;
    const bool match = j < n && (int64_t)t == ids[(size_t)r * ld + j + 1];
    const unsigned long long miss = __ballot(!match);                       // lanes >= n miss: never zero
    const int a = (int)__ffsll((long long)miss) - 1;
    const int covered = a < n ? a + 1 : n;
    if (j < covered) {
        ids[(size_t)r * ld + j + 1] = t;
        if (t == sep_id) atomicAdd(&sep_cnt[j], 1);
        if (LP)
            lp_out[(size_t)r * ld_lp + j] = __int_as_float(__hip_atomic_load(lp_tok + r * n + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    }
    if (j == 0) {
        len[r] = 1 + covered;
        if (host_rows) host_rows[r] = a;
        __hip_atomic_store(row_res + 2 * r, covered, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(row_res + 2 * r + 1, a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                         // (the wave's stores and atomics have reached memory)
    int last_row = 0;
    if (j == 0) {
        const unsigned old = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_row = old == (unsigned)B - 1;
        if (last_row) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (!__shfl(last_row, 0)) return;
    int cmin = n, cmax = 0, asum = 0;
    for (int q = j; q < B; q += 64) {
        const int c = __hip_atomic_load(row_res + 2 * q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cmin = min(cmin, c);
        cmax = max(cmax, c);
        asum += __hip_atomic_load(row_res + 2 * q + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        cmin = min(cmin, __shfl_xor(cmin, o));
        cmax = max(cmax, __shfl_xor(cmax, o));
        asum += __shfl_xor(asum, o);
    }
    const int cnt = j < cmin ? __hip_atomic_load(sep_cnt + j, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : -1;
    const bool fired = __ballot(j < cmin && cnt == B) != 0ull;
    if (j == 0) { host[0] = cmin; host[1] = cmax; host[2] = asum; host[3] = fired ? 1 : 0; }
}

// ---- scoring of given captions (gitcap_score; kernels.h: launch_score_final) ---------------------------------------------------
// the one statement of which positions count: target y = ids[r][j + 1] inside the vocabulary, not ignore_id, in front of lengths[r]
__device__ __forceinline__ bool score_counted(const int64_t* __restrict__ ids, int ld_ids, const int32_t* __restrict__ lengths,
                                              int64_t ignore_id, int V, int r, int j) {
    const int64_t y = ids[(size_t)r * ld_ids + j + 1];
    return y >= 0 && y < V && y != ignore_id && (!lengths || j + 1 < lengths[r]);
}
// One workgroup per (row r, position j < T - 1) over the partials of head row m = r * T + j: the row's winner and its
// log-probability exactly as argmax_final_kernel<.., true> forms them (argmax_partials_waves / _pick, lp_partials: same tie rule,
// same summation order, same bits), and the given token's: (its logit - M) + the winner's log-probability, i.e.
// (y_t - M) - log(total).  A -inf target logit gives -inf outright (an all -inf row has M = -inf: never -inf - -inf).  The
// target logit of an ignored position was never written and is not used.
__global__ __launch_bounds__(256) void score_final_kernel(const float* __restrict__ val, const int* __restrict__ idx,
                                                          const float* __restrict__ psum, int ntiles, const float* __restrict__ tgt_logit,
                                                          const int64_t* __restrict__ ids, int ld_ids, int T,
                                                          const int32_t* __restrict__ lengths, int64_t ignore_id, int V,
                                                          float* __restrict__ lp_out, int ld_lp, int64_t* __restrict__ top1_ids,
                                                          float* __restrict__ top1_lp) {
    __shared__ float sv[4];
    __shared__ int si[4];
    __shared__ float vmax, ss[4];
    const int r = blockIdx.x / (T - 1), j = blockIdx.x - r * (T - 1), tid = threadIdx.x;
    const size_t m = (size_t)r * T + j, base = m * ntiles;
    float best;
    int bi;
    argmax_partials_waves(val, idx, base, ntiles, sv, si, best, bi);
    if (tid == 0) bi = argmax_partials_pick(sv, si, best, bi, &vmax);
    __syncthreads();
    const float lp1 = lp_partials(val, psum, base, ntiles, vmax, ss);
    if (tid != 0) return;
    if (top1_ids) top1_ids[blockIdx.x] = bi;
    if (top1_lp) top1_lp[blockIdx.x] = lp1;
    float lp = 0.f;
    if (score_counted(ids, ld_ids, lengths, ignore_id, V, r, j)) {
        const float yt = tgt_logit[m];
        lp = yt == -INFINITY ? -INFINITY : (yt - vmax) + lp1;
    }
    lp_out[(size_t)r * ld_lp + j] = lp;
}
// row_sum[r] = the counted positions' lp, added in ascending position order by one thread; row_cnt[r] = their number
__global__ __launch_bounds__(64) void score_rows_kernel(const float* __restrict__ lp, int ld_lp, const int64_t* __restrict__ ids, int ld_ids,
                                                        int rows, int T, const int32_t* __restrict__ lengths, int64_t ignore_id, int V,
                                                        float* __restrict__ row_sum, int32_t* __restrict__ row_cnt) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= rows) return;
    float sum = 0.f;
    int cnt = 0;
    for (int j = 0; j + 1 < T; ++j)
        if (score_counted(ids, ld_ids, lengths, ignore_id, V, r, j)) { sum += lp[(size_t)r * ld_lp + j]; ++cnt; }
    if (row_sum) row_sum[r] = sum;
    if (row_cnt) row_cnt[r] = cnt;
}

// ---- teacher-student divergence (gitcap_distill; kernels.h: launch_distill_final) -------------------------------------------------
// One workgroup per (row r, position j < T) over the seven partials of head row m = r * T + j (skinny.hip: skinny_head_dual_kernel).
// Each model's winner, maximum M, merged sum Z and -log Z exactly as score_final_kernel forms them (argmax_partials_waves / _pick,
// lp_partials: same tie rule, same summation order, same bits).  The cross term re-centred with the tile maxima,
//     C = sum_tiles e^(t_max - Mt) (cross + t_sum ((t_max - Mt) - (s_max - Ms))),
// over the tiles with t_max > -inf in lp_partials' order (thread tid takes tiles tid, tid + 256, .. ascending, the xor butterfly,
// waves 0 .. 3); a tile whose cross is +inf (the teacher puts mass where the student has -inf) adds +inf outright: its s_max may be
// -inf, and neither 0 * inf nor -inf - -inf is ever formed.  kl = (C / Zt + -log Zt) - -log Zs; a negative value no further from 0
// than DISTILL_CLAMP (the two logs' share of the rounding bound, tests/distill_reference.py) becomes 0, anything else is left to show.
// A row the teacher gives no column at all (Mt = -inf) has kl 0.
__global__ __launch_bounds__(256) void distill_final_kernel(DistillPartials p, int ntiles, const float* __restrict__ t_logit,
                                                            const float* __restrict__ s_logit, const int64_t* __restrict__ ids, int ld_ids,
                                                            int T, const int32_t* __restrict__ lengths, int64_t ignore_id, int V, DistillOut o) {
    __shared__ float svt[4], svs[4], sst[4], sss[4], sc[4];
    __shared__ int sit[4], sis[4];
    __shared__ float vmax_t, vmax_s;
    const int r = blockIdx.x / T, j = blockIdx.x - r * T, tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * ntiles;
    float best, zt = 0.f, zs = 0.f;
    int bt, bs;
    argmax_partials_waves(p.t_max, p.t_idx, base, ntiles, svt, sit, best, bt);
    if (tid == 0) bt = argmax_partials_pick(svt, sit, best, bt, &vmax_t);
    argmax_partials_waves(p.s_max, p.s_idx, base, ntiles, svs, sis, best, bs);      // (its barrier publishes vmax_t)
    if (tid == 0) bs = argmax_partials_pick(svs, sis, best, bs, &vmax_s);
    const float lpt = lp_partials(p.t_max, p.t_sum, base, ntiles, vmax_t, sst, &zt);
    __syncthreads();                                                                // vmax_s
    const float lps = lp_partials(p.s_max, p.s_sum, base, ntiles, vmax_s, sss, &zs);
    const float Mt = vmax_t, Ms = vmax_s;
    float c = 0.f;
    if (Mt != -INFINITY) {
        for (int i0 = tid; i0 < ntiles; i0 += 256 * 8) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int i = i0 + 256 * u;
                if (i < ntiles) {
                    const float tm = p.t_max[base + i];
                    if (tm != -INFINITY) {
                        const float cr = p.cross[base + i];
                        c += cr == INFINITY ? INFINITY : __expf(tm - Mt) * (cr + p.t_sum[base + i] * ((tm - Mt) - (p.s_max[base + i] - Ms)));
                    }
                }
            }
        }
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off);
    if ((tid & 63) == 0) sc[tid >> 6] = c;
    __syncthreads();
    if (tid != 0) return;
    const bool live = !lengths || j < lengths[r];
    float kl = 0.f;
    if (live && Mt != -INFINITY) {
        const float C = ((sc[0] + sc[1]) + sc[2]) + sc[3];
        kl = (C / zt + lpt) - lps;
        if (kl < 0.f && kl >= -DISTILL_CLAMP) kl = 0.f;
    }
    o.kl[(size_t)r * o.ld_kl + j] = kl;
    if (o.t_top1) o.t_top1[blockIdx.x] = bt;
    if (o.s_top1) o.s_top1[blockIdx.x] = bs;
    if (o.agree) o.agree[blockIdx.x] = bt == bs ? 1 : 0;
    if (j + 1 < T && (o.t_lp || o.s_lp)) {
        const bool cnt = score_counted(ids, ld_ids, lengths, ignore_id, V, r, j);
        float a = 0.f, b = 0.f;
        if (cnt && o.t_lp) { const float y = t_logit[blockIdx.x]; a = y == -INFINITY ? -INFINITY : (y - Mt) + lpt; }
        if (cnt && o.s_lp) { const float y = s_logit[blockIdx.x]; b = y == -INFINITY ? -INFINITY : (y - Ms) + lps; }
        if (o.t_lp) o.t_lp[(size_t)r * o.ld_lp + j] = a;
        if (o.s_lp) o.s_lp[(size_t)r * o.ld_lp + j] = b;
    }
}
// row_kl_sum[r] = the counted positions' kl, added in ascending position order by one thread; row_cnt[r] = their number
__global__ __launch_bounds__(64) void distill_rows_kernel(const float* __restrict__ kl, int ld_kl, int rows, int T,
                                                          const int32_t* __restrict__ lengths, float* __restrict__ row_sum,
                                                          int32_t* __restrict__ row_cnt) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r >= rows) return;
    const int n = lengths ? min(max(lengths[r], 0), T) : T;
    float sum = 0.f;
    for (int j = 0; j < n; ++j) sum += kl[(size_t)r * ld_kl + j];
    if (row_sum) row_sum[r] = sum;
    if (row_cnt) row_cnt[r] = n;
}

// ---- beam candidates: top-K of (log_softmax(logits[b*beams+j]) + beam_score[b*beams+j]) over j, v ----
// Replaces log_softmax (:557) + add (:561) + view + topk (:563-565) of the reference search loop
// (src/models/model.py); flat index = j*V + v, sorted descending, ties by smaller flat index.
// Two launches (a single workgroup per clip scanned beams x V = 122 K logits three times: 371 us at the configs[4] shape,
// a quarter of its search loop):
//   chunks: one workgroup per (row, 2048-logit chunk): chunk max, sum of exp(x - max), and the chunk's top K by value
//           (inside a row the order by logit IS the order by score);
//   merge:  one wave per clip: log-sum-exp of every row from the chunk statistics (fixed order), score of every candidate,
//           top K of the beams x chunks x K candidates.  The global top K is a subset of the per-chunk top K's: exact.
// Both keep a descending list tv / ti of KMAX (value, id) per thread and take K rounds of arg-max over the list heads, the owner
// of a round's winner popping it.  The insert, the arg-max round and the pop are written out in both kernels: as shared inline
// functions they compile to a different schedule of both (docs/LAB_NOTEBOOK.md, round 15).
constexpr int BT_CHUNK = 2048;

// PEN: the chunk kernel under a repetition penalty (model.py:522-531): every logit whose column occurs in the row's prefix
// ids[row * ld_ids + 0 .. cur_len - 1] (CLS included) is rewritten x < 0 ? x * rp : x / rp before the chunk statistics and the
// chunk's top K are taken, so the log-softmax is that of the penalised row.  A column is penalised once however often it occurs:
// the prefix sets bits of a 2048-bit LDS map of the chunk, every thread then tests the bits of its 8 columns.  An id outside
// [0, V) sets no bit.  -inf stays -inf; plain IEEE fp32 multiply / divide.  The penalty's arguments come last and are empty
// without it: the plain instantiation has the bit map, its two barriers and the rewrite compiled out.
template <bool PEN> struct BeamPenalty {};
template <> struct BeamPenalty<true> { const int64_t* prefix_ids; int ld_ids, cur_len; float rp; };

// BAN (constrained decoding; kernels.h: HeadBan): every thread tests the mask bits of its 8 columns -- row `row` of the mask, one
// uint16 word per 16 columns -- and a banned column is -inf before the penalty (under which -inf stays -inf: the order of the two
// is immaterial), the chunk statistics and the chunk's top K.  Combinable with PEN; its arguments are empty without it, like the
// penalty's: the plain instantiations have the test compiled out.
template <bool BAN> struct BeamBan {};
template <> struct BeamBan<true> { const uint16_t* mask; int ld; };

template <int KMAX, bool PEN, bool BAN = false>
__global__ __launch_bounds__(256) void beam_topk_chunks_kernel(const float* __restrict__ logits, int ld, int V, int K, int nch,
                                                               float2* __restrict__ stats, float* __restrict__ cval,
                                                               int* __restrict__ cidx, BeamPenalty<PEN> pen, BeamBan<BAN> ban = BeamBan<BAN>{}) {
    __shared__ float red[4];
    __shared__ int redi[4];
    __shared__ unsigned seen[PEN ? BT_CHUNK / 32 : 1];
    const int row = blockIdx.x / nch, c = blockIdx.x - row * nch;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float* src = logits + (size_t)row * ld;
    if constexpr (PEN) {
        if (tid < BT_CHUNK / 32) seen[tid] = 0u;
        __syncthreads();
        for (int t = tid; t < pen.cur_len; t += 256) {
            const int64_t id = pen.prefix_ids[(size_t)row * pen.ld_ids + t];
            if (id >= 0 && id < (int64_t)V) {
                const int rel = (int)id - c * BT_CHUNK;
                if (rel >= 0 && rel < BT_CHUNK) atomicOr(&seen[rel >> 5], 1u << (rel & 31));
            }
        }
        __syncthreads();
    }
    float x[8];
    float m = -INFINITY;
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const int rel = q * 256 + tid;
        const int i = c * BT_CHUNK + rel;
        float v = i < V ? src[i] : -INFINITY;
        if constexpr (BAN) {
            if (i < V && ((ban.mask[(size_t)row * ban.ld + (i >> 4)] >> (i & 15)) & 1u)) v = -INFINITY;
        }
        if constexpr (PEN) {
            if ((seen[rel >> 5] >> (rel & 31)) & 1u) v = v < 0.f ? v * pen.rp : v / pen.rp;
        }
        x[q] = v;
        m = fmaxf(m, v);
    }
    m = wave_max(m);
    if (lane == 0) red[wid] = m;
    __syncthreads();
    m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    __syncthreads();
    float sum = 0.f;
#pragma unroll
    for (int q = 0; q < 8; ++q) sum += x[q] == -INFINITY ? 0.f : expf(x[q] - m);      // (a chunk of -inf only: m = -inf, sum = 0)
    sum = wave_sum(sum);
    if (lane == 0) red[wid] = sum;
    __syncthreads();
    if (tid == 0) stats[blockIdx.x] = float2{m, (red[0] + red[1]) + (red[2] + red[3])};
    __syncthreads();
    float tv[KMAX];
    int ti[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) { tv[k] = -INFINITY; ti[k] = 0x7fffffff; }
#pragma unroll
    for (int q = 0; q < 8; ++q) {                                        // ascending ids per thread: strict > keeps the earlier one
        float v = x[q];
        int id = c * BT_CHUNK + q * 256 + tid;
        if (v > tv[KMAX - 1]) {
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (v > tv[k]) { const float fv = tv[k]; const int fi = ti[k]; tv[k] = v; ti[k] = id; v = fv; id = fi; }
        }
    }
    for (int k = 0; k < K; ++k) {                                        // K rounds of block arg-max over the list heads
        float bv = tv[0];
        int bi = ti[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(bv, o);
            const int i2 = __shfl_xor(bi, o);
            if (v2 > bv || (v2 == bv && i2 < bi)) { bv = v2; bi = i2; }
        }
        if (lane == 0) { red[wid] = bv; redi[wid] = bi; }
        __syncthreads();
        bv = red[0]; bi = redi[0];
        for (int w = 1; w < 4; ++w)
            if (red[w] > bv || (red[w] == bv && redi[w] < bi)) { bv = red[w]; bi = redi[w]; }
        if (tid == 0) { cval[(size_t)blockIdx.x * K + k] = bv; cidx[(size_t)blockIdx.x * K + k] = bi; }
        if (ti[0] == bi && bi != 0x7fffffff) {                           // the owner pops its head
#pragma unroll
            for (int q = 0; q + 1 < KMAX; ++q) { tv[q] = tv[q + 1]; ti[q] = ti[q + 1]; }
            tv[KMAX - 1] = -INFINITY; ti[KMAX - 1] = 0x7fffffff;
        }
        __syncthreads();
    }
}

template <int KMAX>
__global__ __launch_bounds__(64) void beam_topk_merge_kernel(const float2* __restrict__ stats, const float* __restrict__ cval,
                                                             const int* __restrict__ cidx, const float* __restrict__ beam_scores,
                                                             int beams, int V, int K, int nch, float* __restrict__ out_scores,
                                                             int* __restrict__ out_idx) {
    __shared__ float add[16];
    const int b = blockIdx.x, lane = threadIdx.x;
    // (the chunk statistics of four beams per round trip, the candidates eight per round trip: requested together, then used --
    // one at a time every load was a round trip of its own, 30 of them for 4 beams x 30 chunks x 8 candidates)
    for (int j0 = 0; j0 < beams; j0 += 4) {
        float2 st4[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) st4[u] = stats[(size_t)(b * beams + min(j0 + u, beams - 1)) * nch + min(lane, nch - 1)];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
        const int j = j0 + u;
        if (j >= beams) break;
        const float2 st = lane < nch ? st4[u] : float2{-INFINITY, 0.f};  // log-sum-exp of row j from its chunks (nch <= 64)
        const float M = wave_max(st.x);
        const float S = wave_sum(st.y == 0.f ? 0.f : st.y * expf(st.x - M));
        if (lane == 0) add[j] = beam_scores[b * beams + j] - (M + logf(S));
        }
    }
    __syncthreads();
    float tv[KMAX];
    int ti[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; ++k) { tv[k] = -INFINITY; ti[k] = 0x7fffffff; }
    const int per_row = nch * K, total = beams * per_row;
    for (int t0 = lane; t0 < total; t0 += 64 * 8) {
        int ci8[8];
        float cv8[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const size_t at = (size_t)(b * beams) * per_row + min(t0 + 64 * u, total - 1);
            ci8[u] = cidx[at];
            cv8[u] = cval[at];
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int t = t0 + 64 * u;
            if (t >= total || ci8[u] == 0x7fffffff) continue;            // past the end / an empty slot of a short last chunk
            const int j = t / per_row;
            float v = cv8[u] + add[j];
            int id = j * V + ci8[u];
#pragma unroll
            for (int k = 0; k < KMAX; ++k)
                if (v > tv[k] || (v == tv[k] && id < ti[k])) { const float fv = tv[k]; const int fi = ti[k]; tv[k] = v; ti[k] = id; v = fv; id = fi; }
        }
    }
    for (int k = 0; k < K; ++k) {                                        // K rounds of wave arg-max over the list heads
        float bv = tv[0];
        int bi = ti[0];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(bv, o);
            const int i2 = __shfl_xor(bi, o);
            if (v2 > bv || (v2 == bv && i2 < bi)) { bv = v2; bi = i2; }
        }
        if (lane == 0) { out_scores[b * K + k] = bv; out_idx[b * K + k] = bi; }
        if (ti[0] == bi && bi != 0x7fffffff) {                           // the owner pops its head
#pragma unroll
            for (int q = 0; q + 1 < KMAX; ++q) { tv[q] = tv[q + 1]; ti[q] = ti[q + 1]; }
            tv[KMAX - 1] = -INFINITY; ti[KMAX - 1] = 0x7fffffff;
        }
    }
}

// ---- sampled candidates: the do_sample branch of the search (model.py:532-554) ----------------------------------------------------
// One 1024-thread workgroup per row, the row in LDS (V fp32 of dynamic LDS, V <= 32768: 128 of the CU's 160 KB); thread t owns columns
// t, t + 1024, ... and is the only one to touch them, so the row needs no barrier of its own and the accesses are conflict free.
// Rows are few -- 64 at the configs[4] shape -- but every decision below needs a statistic of the WHOLE row, and the bisections need
// ~64 of them in sequence: chunk workgroups (beam_topk's shape) would pay a grid-wide hand-off per statistic, one workgroup pays a
// barrier.  Registers cannot hold the row (32 columns per thread beside the filter's temporaries do not fit the 128 VGPRs of a
// 16-wave workgroup); LDS does, and the loops over it stay rolled.
//   row:    raw logit, penalised when its column occurs in the row's prefix (the rule of beam_topk_chunks_kernel<.., true>: once per
//           column, ids outside [0, V) match nothing), divided by the temperature when it is not 1, -0 made +0.
//   top_k:  k' = min(max(top_k, 2), V); T = the k'-th largest value, found by bisection on the order-preserving integer image of
//           fp32 (32 counting passes, integer sums); columns below T become -inf, ties with T stay.
//   top_p:  on the softmax of that row: column v stays iff fewer than 3 columns are strictly greater or the mass of the strictly
//           greater columns is <= top_p.  Both conditions are monotone in the value, so the kept set is {x >= t*}; t* by bisection,
//           each pass one count and one mass sum.  Columns of equal value share one fate (the oracle's choice among equal values is
//           the order its sort leaves them in, which is no contract).  -inf is never kept.
//   draw:   u_v from Philox4x32-10, key (seed_lo, seed_hi), counter (v / 4, row, cur_len, 0), lane v % 4: u = ((x >> 8) + 0.5) 2^-24.
//           With n = x >> 8: n < 2^23 makes u exact in fp32 and E = -logf(u); otherwise 1 - u = ((2^24 - 1 - n) + 0.5) 2^-24 is exact
//           and E = -log1pf(-(1 - u)) (u itself would round to 1 at the top of the range).  key_v = z_v - logf(E_v) over the kept
//           columns, written over the row; the pn largest keys, descending, ties to the smaller column, are the draws: sampling
//           without replacement.  The logit of a drawn column is computed again from the raw row (the same operations: the same bits).
//   score:  (z_w - logZ) + beam_score[row], logZ = M + logf(sum of expf(z - M) over the kept columns).
// Every sum is a per-thread sum in column order, a wave butterfly and 16 partials added in wave order: the same bits every run.
// Candidate p = j * pn + d of clip b is draw d of row b * beams + j, flat index (p % beams) * V + word (model.py:549-552 tiles the
// beam offsets over the row; kept as the host operator has it).  A row with fewer than pn kept columns fills the rest with the
// sentinel (-inf, 0x7fffffff), which beam_step_nbest_kernel<true> passes over.
constexpr int SR_THREADS = 1024, SR_WAVES = SR_THREADS / 64, SR_MAX_V = 32768;

__device__ __forceinline__ unsigned f32_ord(float x) {
    const unsigned b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ unsigned philox4x32_10_lane(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, int lane) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const unsigned hi0 = __umulhi(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
        const unsigned hi1 = __umulhi(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
        c0 = hi1 ^ c1 ^ k0; c1 = lo1; c2 = hi0 ^ c3 ^ k1; c3 = lo0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return lane == 0 ? c0 : lane == 1 ? c1 : lane == 2 ? c2 : c3;
}

// column i of the row as the filter sees it: penalty, temperature, -0 -> +0 (one integer image per value)
// banrow (BAN form; nullable): the row of the ban mask (kernels.h: HeadBan) -- a banned column is -inf before everything else
__device__ __forceinline__ float sr_logit(const float* __restrict__ src, int i, const int64_t* __restrict__ pre, int cur_len, float rp,
                                          float temperature, const uint16_t* __restrict__ banrow = nullptr) {
    float v = src[i];
    if (banrow && ((banrow[i >> 4] >> (i & 15)) & 1u)) v = -INFINITY;
    if (rp != 1.0f) {
        bool hit = false;
        for (int t = 0; t < cur_len; ++t) hit |= pre[t] == (int64_t)i;
        if (hit) v = v < 0.f ? v * rp : v / rp;
    }
    if (temperature != 1.0f) v = v / temperature;
    if (v == 0.f) v = 0.f;
    return v;
}

struct SrRed { float f[2][SR_WAVES]; int i[2][SR_WAVES]; };

// block sums of (f, i) in a fixed order; one barrier per call (the two halves of SrRed alternate)
__device__ __forceinline__ void sr_block_sum(SrRed& r, int& phase, float& f, int& i) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    f = wave_sum(f);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) i += __shfl_xor(i, o);
    if (lane == 0) { r.f[phase][wid] = f; r.i[phase][wid] = i; }
    __syncthreads();
    float fs = 0.f;
    int is = 0;
#pragma unroll
    for (int w = 0; w < SR_WAVES; ++w) { fs += r.f[phase][w]; is += r.i[phase][w]; }
    f = fs; i = is;
    phase ^= 1;
}

template <bool BAN>
__global__ __launch_bounds__(SR_THREADS) void sample_rows_kernel(const float* __restrict__ logits, int ld, int V,
                                                                 const float* __restrict__ beam_scores,
                                                                 const int64_t* __restrict__ prefix_ids, int ld_ids, int cur_len, float rp,
                                                                 int beams, int pn, float temperature, int top_k, float top_p,
                                                                 unsigned seed_lo, unsigned seed_hi, float* __restrict__ out_scores,
                                                                 int* __restrict__ out_idx, int* __restrict__ kept_out,
                                                                 float* __restrict__ logz_out, BeamBan<BAN> ban) {
    extern __shared__ float sr_row[];                                    // [V]: the row, later its keys
    __shared__ SrRed red;
    __shared__ float s_bk[2][SR_WAVES];
    __shared__ int s_bi[2][SR_WAVES];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const float* src = logits + (size_t)row * ld;
    const int64_t* pre = rp != 1.0f ? prefix_ids + (size_t)row * ld_ids : nullptr;
    const uint16_t* banrow = nullptr;                                    // BAN: the bits are tested before temperature and filter
    if constexpr (BAN) banrow = ban.mask + (size_t)row * ban.ld;
    int phase = 0;
    float m = -INFINITY;
    for (int i = tid; i < V; i += SR_THREADS) {
        const float v = sr_logit(src, i, pre, cur_len, rp, temperature, banrow);
        sr_row[i] = v;
        m = fmaxf(m, v);
    }
    m = wave_max(m);
    if (lane == 0) red.f[phase][wid] = m;
    __syncthreads();
    m = red.f[phase][0];
#pragma unroll
    for (int w = 1; w < SR_WAVES; ++w) m = fmaxf(m, red.f[phase][w]);
    phase ^= 1;

    if (top_k > 0) {
        const int kk = min(max(top_k, 2), V);
        unsigned T = 0u;
        for (int bit = 31; bit >= 0; --bit) {
            const unsigned cand = T | (1u << bit);
            int c = 0;
            float unused = 0.f;
            for (int i = tid; i < V; i += SR_THREADS) c += f32_ord(sr_row[i]) >= cand;
            sr_block_sum(red, phase, unused, c);
            if (c >= kk) T = cand;
        }
        for (int i = tid; i < V; i += SR_THREADS)
            if (f32_ord(sr_row[i]) < T) sr_row[i] = -INFINITY;
    }

    unsigned tstar = 0u;
    if (top_p < 1.0f) {
        float Z = 0.f;
        int unused = 0;
        for (int i = tid; i < V; i += SR_THREADS) { const float x = sr_row[i]; Z += x == -INFINITY ? 0.f : expf(x - m); }
        sr_block_sum(red, phase, Z, unused);
        const float lim = top_p * Z;
        unsigned L = 0u;
        bool all = false;
        for (int it = -1; it < 32; ++it) {                               // f(t) = fewer than 3 above t, or their mass <= top_p Z
            const unsigned cand = it < 0 ? 0u : (L | (1u << (31 - it)));
            int c = 0;
            float mass = 0.f;
            for (int i = tid; i < V; i += SR_THREADS) {
                const float x = sr_row[i];
                const bool above = f32_ord(x) > cand;
                c += above;
                mass += above && x != -INFINITY ? expf(x - m) : 0.f;
            }
            sr_block_sum(red, phase, mass, c);
            const bool ok = c < 3 || mass <= lim;
            if (it < 0) { if (ok) { all = true; break; } }
            else if (!ok) L = cand;
        }
        tstar = all ? 0u : L + 1u;                                       // the smallest t with f(t): L is the largest without
    }

    float S = 0.f;
    int kept = 0;
    for (int i = tid; i < V; i += SR_THREADS) {
        const float x = sr_row[i];
        const bool keep = x != -INFINITY && f32_ord(x) >= tstar;
        kept += keep;
        S += keep ? expf(x - m) : 0.f;
        float k = -INFINITY;
        if (keep) {
            const unsigned n = philox4x32_10_lane((unsigned)i >> 2, (unsigned)row, (unsigned)cur_len, 0u, seed_lo, seed_hi, i & 3) >> 8;
            const float E = n < (1u << 23) ? -logf(((float)n + 0.5f) * 0x1p-24f)
                                           : -log1pf(-(((float)((1u << 24) - 1u - n) + 0.5f) * 0x1p-24f));
            k = x - logf(E);
        }
        sr_row[i] = k;                                                   // the row becomes its keys
    }
    sr_block_sum(red, phase, S, kept);
    const float logZ = m + logf(S);
    if (tid == 0) {
        if (kept_out) kept_out[row] = kept;
        if (logz_out) logz_out[row] = logZ;
    }

    const int b = row / beams, j = row - b * beams, K = beams * pn;
    for (int d = 0; d < pn; ++d) {
        float bk = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = tid; i < V; i += SR_THREADS) {                      // ascending columns: strict > keeps the smaller
            const float k = sr_row[i];
            if (k > bk) { bk = k; bi = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float k2 = __shfl_xor(bk, o);
            const int i2 = __shfl_xor(bi, o);
            if (k2 > bk || (k2 == bk && i2 < bi)) { bk = k2; bi = i2; }
        }
        const int ph = d & 1;
        if (lane == 0) { s_bk[ph][wid] = bk; s_bi[ph][wid] = bi; }
        __syncthreads();
        bk = s_bk[ph][0]; bi = s_bi[ph][0];
#pragma unroll
        for (int w = 1; w < SR_WAVES; ++w)
            if (s_bk[ph][w] > bk || (s_bk[ph][w] == bk && s_bi[ph][w] < bi)) { bk = s_bk[ph][w]; bi = s_bi[ph][w]; }
        const bool none = bi == 0x7fffffff;
        if (tid == 0) {
            const int p = j * pn + d;
            out_scores[(size_t)b * K + p] = none ? -INFINITY : (sr_logit(src, bi, pre, cur_len, rp, temperature, banrow) - logZ) + beam_scores[row];
            out_idx[(size_t)b * K + p] = none ? 0x7fffffff : (p % beams) * V + bi;
        }
        if (!none && (bi & (SR_THREADS - 1)) == tid) sr_row[bi] = -INFINITY;    // the owner retires the drawn column
    }
}

// ---- ban mask of constrained decoding (gitcap_attach_constraints; kernels.h: launch_ban_mask) -------------------------------------
// One workgroup per row.  The row's bitmap is built in LDS (32-bit words, V <= 131072: 16 KB) -- cleared, a barrier, the three rules
// set their bits with LDS atomics, a barrier -- and then EVERY 32-bit word of the row's ld_mask / 2 is stored, the ones behind
// ceil(V / 16) as 0: the result does not depend on what the buffer held (it is reused every step) and needs no global atomic.
// A uint16 word c >> 4, bit c & 15 of the mask is bit c & 31 of 32-bit word c >> 5 (little endian): the same bytes.
//   n-gram (n >= 1; HF NoRepeatNGramLogitsProcessor): thread i <= cur_len - n compares prefix[i .. i + n - 2] with the last n - 1
//           tokens prefix[cur_len - n + 1 .. cur_len - 1] as int64 values and bans prefix[i + n - 1]; nothing while cur_len < n;
//   length: sep_id while cur_len < min_length (HF MinLengthLogitsProcessor);   suppress: the listed ids.
// An id outside [0, V) sets no bit, so the bits of the last word beyond V stay 0.
constexpr int BM_MAX_V = 131072;

__global__ __launch_bounds__(256) void ban_mask_kernel(const int64_t* __restrict__ ids, int ld_ids, int cur_len, int n, int min_length,
                                                       int sep_id, const int32_t* __restrict__ suppress, int n_suppress, int V,
                                                       unsigned* __restrict__ mask32, int ld32) {
    __shared__ unsigned bits[BM_MAX_V / 32];
    const int row = blockIdx.x, tid = threadIdx.x;
    const int nw = (V + 31) >> 5;
    for (int w = tid; w < nw; w += 256) bits[w] = 0u;
    __syncthreads();
    const int64_t* pre = ids + (size_t)row * ld_ids;
    auto ban = [&](int64_t id) {
        if (id >= 0 && id < (int64_t)V) atomicOr(&bits[(int)id >> 5], 1u << ((int)id & 31));
    };
    if (n >= 1) {
        for (int i = tid; i <= cur_len - n; i += 256) {
            bool eq = true;
            for (int j = 0; j + 1 < n; ++j) eq &= pre[i + j] == pre[cur_len - n + 1 + j];
            if (eq) ban(pre[i + n - 1]);
        }
    }
    if (tid == 0 && cur_len < min_length) ban((int64_t)sep_id);
    for (int k = tid; k < n_suppress; k += 256) ban((int64_t)suppress[k]);
    __syncthreads();
    unsigned* out = mask32 + (size_t)row * ld32;
    for (int w = tid; w < ld32; w += 256) out[w] = w < nw ? bits[w] : 0u;
}

// ---- device-side beam bookkeeping: one step of GeneratorWithBeamSearchV2.search (model.py:573-621) -----
// One block per batch element; thread 0 walks the <= 16 sorted candidates exactly like the reference's
// Python loop (finished hypotheses kept n_best = 1: score = sum_logprob / len^length_penalty, :503, :592-594;
// is_done test :576), then the block copies the surviving prefixes into the next id buffer (:620-621).

struct BeamState {
    int64_t* ids[2];          // [B*beams][max_len] prefixes, double buffered
    float* beam_scores;       // [B*beams]
    int64_t* words;           // [B*beams] token chosen for the next position (input of the next decoder step)
    int32_t* src_rows;        // [B*beams] row each new beam continues (for the KV reorder)
    int32_t* done;            // [B]
    int32_t* hyp_len;         // [B][n] 0 = an empty slot
    float* hyp_score;         // [B][n]
    int64_t* hyp_ids;         // [B][n][max_len]
};

// A forced step of a prompted search (gitcap_attach_prompt): clip b at cur_len < lengths[b] is not ranked.  Every beam of the clip
// keeps its prefix and appends the prompt's token, src_rows is the identity; beam_scores, done and the hypothesis slots are not
// touched (no is_done test, no hypothesis added), the candidates are not read.  The whole wave; true = the clip was forced.
__device__ __forceinline__ bool beam_step_forced(const BeamState& st, const PromptSel<true>& pr, const int b, const int beams,
                                                 const int cur_len, const int max_len, const int cur) {
    if (cur_len >= prompt_len(pr.lengths, b, pr.max_len)) return false;
    const int64_t* ids_old = st.ids[cur];
    int64_t* ids_new = st.ids[cur ^ 1];
    const int64_t tok = pr.ids[(size_t)b * pr.ld + cur_len];
    for (int j = 0; j < beams; ++j) {
        const int r = b * beams + j;
        for (int t = threadIdx.x; t < cur_len; t += 64) ids_new[(size_t)r * max_len + t] = ids_old[(size_t)r * max_len + t];
        if (threadIdx.x == 0) {
            ids_new[(size_t)r * max_len + cur_len] = tok;
            st.words[r] = tok;
            st.src_rows[r] = r;
        }
    }
    return true;
}

// n = 1: one finished hypothesis per clip in hyp_ids [B][max_len], hyp_score [B], hyp_len [B] (0 = none yet).
// FORCED: clips still inside their prompt take beam_step_forced; <false> is the kernel as it was before it became a template.
template <bool FORCED>
__global__ __launch_bounds__(64) void beam_step_kernel(BeamState st, const float* __restrict__ cand_scores,
                                                       const int* __restrict__ cand_idx, int beams, int K, int V,
                                                       int cur_len, int max_len, int eos, float length_penalty, int cur,
                                                       PromptSel<FORCED> pr) {
    __shared__ int s_src[16];
    __shared__ long long s_word[16];
    const int b = blockIdx.x, tid = threadIdx.x;
    if constexpr (FORCED)
        if (beam_step_forced(st, pr, b, beams, cur_len, max_len, cur)) return;
    const int64_t* ids_old = st.ids[cur];
    int64_t* ids_new = st.ids[cur ^ 1];
    if (tid == 0) {
        const float* cs = cand_scores + (size_t)b * K;
        const int* ci = cand_idx + (size_t)b * K;
        bool done = st.done[b] != 0;
        if (!done && st.hyp_len[b] > 0)                                   // BeamHypotheses.is_done(best_sum_logprobs)
            done = st.hyp_score[b] >= cs[0] / powf((float)(max_len - 1), length_penalty);
        int kept = 0;
        if (!done) {
            for (int c = 0; c < K && kept < beams; ++c) {
                const int beam_id = ci[c] / V, word = ci[c] - beam_id * V;
                if (word == eos || cur_len + 1 == max_len) {              // finished hypothesis: ids[:cur_len]
                    const float score = cs[c] / powf((float)cur_len, length_penalty);
                    if (st.hyp_len[b] == 0 || score > st.hyp_score[b]) {
                        st.hyp_score[b] = score;
                        st.hyp_len[b] = cur_len;
                        const int64_t* srow = ids_old + (size_t)(b * beams + beam_id) * max_len;
                        for (int t = 0; t < cur_len; ++t) st.hyp_ids[(size_t)b * max_len + t] = srow[t];
                    }
                } else {
                    s_src[kept] = b * beams + beam_id;
                    s_word[kept] = word;
                    st.beam_scores[b * beams + kept] = cs[c];
                    ++kept;
                }
            }
        }
        if (kept < beams) {                                               // done, or the last step: pad (0, eos, row 0)
            for (int j = 0; j < beams; ++j) {
                s_src[j] = 0; s_word[j] = eos;
                st.beam_scores[b * beams + j] = 0.f;
            }
        }
        st.done[b] = done ? 1 : 0;
    }
    __syncthreads();
    for (int j = 0; j < beams; ++j) {
        const int r = b * beams + j, src = s_src[j];
        for (int t = tid; t < cur_len; t += 64) ids_new[(size_t)r * max_len + t] = ids_old[(size_t)src * max_len + t];
        if (tid == 0) {
            ids_new[(size_t)r * max_len + cur_len] = s_word[j];
            st.words[r] = s_word[j];
            st.src_rows[r] = src;
        }
    }
}


// ---- the same bookkeeping with n finished hypotheses per clip (num_keep_best = n, 1 <= n <= 16) ---------------------------------
// BeamHypotheses of the reference's search (model.py:503): hyp_ids [B][n][max_len], hyp_score [B][n], hyp_len [B][n] hold the
// stored hypotheses of a clip in STORAGE ORDER in slots 0 .. cnt - 1 (hyp_len > 0: a hypothesis is at least CLS); slots behind
// them have hyp_len 0.
//   add:     fewer than n stored: append.  Otherwise the stored minimum (the earliest stored among equal minima) is deleted --
//            the slots behind it move down one, as `del list[i]` does -- and the new one is appended, only if its score is
//            strictly greater than that minimum.
//   is_done: false while fewer than n are stored, else min stored score >= best candidate sum / (max_len - 1)^length_penalty.
// One wave per clip.  Thread 0 walks the <= 16 sorted candidates as beam_step_kernel does and posts what to store (s_cmd); the
// wave moves the ids (lane t owns column t of every slot, so the slots of a shift need no barrier between them).  n = 1 never
// gets here: launch_beam_step sends it to beam_step_kernel, which the n-slot kernel does not match for speed (5.7 against 6.0 us
// per call at the configs[4] shape).  SAMPLED: the candidates are draws in no order (sample_rows_kernel): the done test takes the
// maximum of the K scores, sentinel candidates are passed over, and a clip left with 0 < kept < beams live beams pads only the
// missing ones.  <false> has the registers, scratch and occupancy of the kernel before it was a template (profiles/).
// FORCED: as beam_step_kernel's.
template <bool SAMPLED, bool FORCED = false>
__global__ __launch_bounds__(64) void beam_step_nbest_kernel(BeamState st, int n, const float* __restrict__ cand_scores,
                                                             const int* __restrict__ cand_idx, int beams, int K, int V,
                                                             int cur_len, int max_len, int eos, float length_penalty, int cur,
                                                             PromptSel<FORCED> pr) {
    __shared__ int s_src[16];
    __shared__ long long s_word[16];
    __shared__ float s_hs[16];
    __shared__ int s_hl[16];
    __shared__ int s_cnt, s_cmd, s_from;
    __shared__ float s_score;
    const int b = blockIdx.x, tid = threadIdx.x;
    if constexpr (FORCED)
        if (beam_step_forced(st, pr, b, beams, cur_len, max_len, cur)) return;
    const int64_t* ids_old = st.ids[cur];
    int64_t* ids_new = st.ids[cur ^ 1];
    int64_t* hyp = st.hyp_ids + (size_t)b * n * max_len;
    if (tid < n) { s_hs[tid] = st.hyp_score[b * n + tid]; s_hl[tid] = st.hyp_len[b * n + tid]; }
    __syncthreads();
    const float* cs = cand_scores + (size_t)b * K;
    const int* ci = cand_idx + (size_t)b * K;
    bool done = false;
    int kept = 0;
    if (tid == 0) {
        int cnt = 0;
        while (cnt < n && s_hl[cnt] > 0) ++cnt;
        s_cnt = cnt;
        done = st.done[b] != 0;
        if (!done && cnt == n) {                                          // BeamHypotheses.is_done(best_sum_logprobs)
            float worst = s_hs[0];
            for (int i = 1; i < n; ++i) worst = fminf(worst, s_hs[i]);
            float best = cs[0];
            if constexpr (SAMPLED)
                for (int c = 1; c < K; ++c) best = fmaxf(best, cs[c]);    // (a sentinel's -inf never wins)
            done = worst >= best / powf((float)(max_len - 1), length_penalty);
        }
    }
    for (int c = 0; c < K; ++c) {
        if (tid == 0) {
            int cmd = -2;                                                 // -2: nothing to store; -1: stop; n: append; e < n: delete slot e, append
            if (done || kept >= beams) {
                cmd = -1;
            } else if (SAMPLED && ci[c] == 0x7fffffff) {                  // a row that ran out of columns: no candidate
            } else {
                const int beam_id = ci[c] / V, word = ci[c] - beam_id * V;
                if (word == eos || cur_len + 1 == max_len) {              // finished hypothesis: ids[:cur_len]
                    const float score = cs[c] / powf((float)cur_len, length_penalty);
                    const int cnt = s_cnt;
                    if (cnt < n) {
                        cmd = n;
                    } else {
                        int e = 0;
                        for (int i = 1; i < n; ++i)
                            if (s_hs[i] < s_hs[e]) e = i;                 // strict <: the earliest stored of equal minima
                        if (score > s_hs[e]) cmd = e;
                    }
                    s_score = score;
                    s_from = b * beams + beam_id;
                } else {
                    s_src[kept] = b * beams + beam_id;
                    s_word[kept] = word;
                    st.beam_scores[b * beams + kept] = cs[c];
                    ++kept;
                }
            }
            s_cmd = cmd;
        }
        __syncthreads();
        const int cmd = s_cmd;
        if (cmd == -1) break;
        if (cmd >= 0) {
            const int cnt = s_cnt;
            const int dst = cmd < n ? cnt - 1 : cnt;
            for (int i = cmd; i < cnt - 1; ++i) {                         // (append: cmd = n >= cnt, no trip)
                const int len = s_hl[i + 1];
                for (int t = tid; t < len; t += 64) hyp[(size_t)i * max_len + t] = hyp[(size_t)(i + 1) * max_len + t];
            }
            const int64_t* srow = ids_old + (size_t)s_from * max_len;
            for (int t = tid; t < cur_len; t += 64) hyp[(size_t)dst * max_len + t] = srow[t];
            __syncthreads();                                              // every lane has read s_hl / s_cnt / s_from
            if (tid == 0) {
                for (int i = cmd; i < cnt - 1; ++i) { s_hs[i] = s_hs[i + 1]; s_hl[i] = s_hl[i + 1]; }
                s_hs[dst] = s_score;
                s_hl[dst] = cur_len;
                s_cnt = dst + 1;
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (kept < beams) {                                               // done, or the last step: pad (0, eos, row 0)
            for (int j = SAMPLED ? kept : 0; j < beams; ++j) {            // (SAMPLED: EOS was drawn often -- only the missing beams)
                s_src[j] = 0; s_word[j] = eos;
                st.beam_scores[b * beams + j] = 0.f;
            }
        }
        st.done[b] = done ? 1 : 0;
    }
    __syncthreads();
    if (tid < n) { st.hyp_score[b * n + tid] = s_hs[tid]; st.hyp_len[b * n + tid] = s_hl[tid]; }
    for (int j = 0; j < beams; ++j) {
        const int r = b * beams + j, src = s_src[j];
        for (int t = tid; t < cur_len; t += 64) ids_new[(size_t)r * max_len + t] = ids_old[(size_t)src * max_len + t];
        if (tid == 0) {
            ids_new[(size_t)r * max_len + cur_len] = s_word[j];
            st.words[r] = s_word[j];
            st.src_rows[r] = src;
        }
    }
}

// decoded[b][k] = the stored hypothesis of rank k by descending score (equal scores in storage order) + EOS padding, logprobs[b][k]
// = its score; a rank with no hypothesis is all-EOS with score -1e5 (model.py:653-678).  One workgroup per (clip, slot): it counts
// the slots ranked before its own.  first_decoded / first_logprobs: rank 0 once more, [B][max_len] / [B].  Every output is nullable.
__global__ __launch_bounds__(64) void beam_finish_kernel(BeamState st, int n, int max_len, int eos, int64_t* __restrict__ decoded,
                                                         float* __restrict__ logprobs, int64_t* __restrict__ first_decoded,
                                                         float* __restrict__ first_logprobs) {
    const int b = blockIdx.x, i = blockIdx.y;
    const int len = st.hyp_len[b * n + i];
    const float score = st.hyp_score[b * n + i];
    int rank = i;                                                         // an empty slot: behind every stored one, in slot order
    if (len > 0) {
        rank = 0;
        for (int j = 0; j < n; ++j) {
            if (j == i || st.hyp_len[b * n + j] <= 0) continue;
            const float sj = st.hyp_score[b * n + j];
            rank += sj > score || (sj == score && j < i);
        }
    }
    const int64_t* src = st.hyp_ids + ((size_t)b * n + i) * max_len;
    for (int t = threadIdx.x; t < max_len; t += blockDim.x) {
        const int64_t v = t < len ? src[t] : (int64_t)eos;
        if (decoded) decoded[((size_t)b * n + rank) * max_len + t] = v;
        if (rank == 0 && first_decoded) first_decoded[(size_t)b * max_len + t] = v;
    }
    if (threadIdx.x == 0) {
        const float lp = len > 0 ? score : -1e5f;
        if (logprobs) logprobs[b * n + rank] = lp;
        if (rank == 0 && first_logprobs) first_logprobs[b] = lp;
    }
}

__global__ void beam_init_kernel(BeamState st, int B, int beams, int n, int max_len, int cls) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < B * beams) {
        st.ids[0][(size_t)r * max_len] = cls;
        st.words[r] = cls;
        st.beam_scores[r] = (r % beams == 0) ? 0.f : -1e9f;                 // model.py:508-509
        st.src_rows[r] = r;
    }
    if (r < B) st.done[r] = 0;
    if (r < B * n) { st.hyp_len[r] = 0; st.hyp_score[r] = 0.f; }
}

// steps_out = number of generated columns that are valid under the stop rule
__global__ void finish_steps_kernel(const int32_t* sep_cnt, int rows, int max_len, int stop, int32_t* steps_out) {
    int steps = max_len;
    if (stop == 1) {
        for (int t = 0; t < max_len; ++t)
            if (sep_cnt[t] == rows) { steps = t + 1; break; }
    }
    *steps_out = steps;
}

__global__ void fill_i64_kernel(int64_t* p, int ld, int rows, int64_t v) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < rows) p[(size_t)r * ld] = v;
}

// the start of a prompted greedy loop: p[r][0 .. lengths[r] - 1] = prompt[r][the same] (lengths clamped to [1, max_len])
__global__ void fill_prompt_kernel(int64_t* p, int ld, int rows, const int64_t* __restrict__ prompt, int ld_prompt,
                                   const int32_t* __restrict__ lengths, int max_len) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = i / max_len, j = i - r * max_len;
    if (r < rows && j < prompt_len(lengths, r, max_len)) p[(size_t)r * ld + j] = prompt[(size_t)r * ld_prompt + j];
}

// dst[l][r][t][:] = src[l][src_rows[r]][t][:] for t < t_len, every layer l = blockIdx.y in one launch
// (text K/V rows, `width` bf16 per position, `layer_stride` elements between layers)
__global__ void gather_txt_rows_kernel(const bf16_t* __restrict__ src, bf16_t* __restrict__ dst,
                                       const int32_t* __restrict__ src_rows, int t_len, int Tmax, int width, size_t layer_stride) {
    const int r = blockIdx.x, sr = src_rows[r];
    const int n8 = t_len * width / 8;
    const uint4* s = (const uint4*)(src + blockIdx.y * layer_stride + (size_t)sr * Tmax * width);
    uint4* d = (uint4*)(dst + blockIdx.y * layer_stride + (size_t)r * Tmax * width);
    for (int i = threadIdx.x; i < n8; i += blockDim.x) d[i] = s[i];
}

}  // namespace

hipError_t launch_layernorm(const LnArgs& a, hipStream_t s) {
    if (a.rows <= 0 || a.D % 4 || a.D > 1024) return hipErrorInvalidValue;
    const int grid = (a.rows + 3) / 4;
    const int nv = (a.D + 255) / 256;
    const bool canon = a.D == 64 || a.D == 128 || a.D == 256 || a.D == 512 || a.D == 768 || a.D == 1024;
    if (a.gamma2 && (!canon || !a.beta2 || !a.out_bf16)) return hipErrorInvalidValue;
    switch (nv * 2 + (canon ? 1 : 0)) {
        case 2: hipLaunchKernelGGL((layernorm_kernel<1, false>), dim3(grid), dim3(256), 0, s, a); break;
        case 3: hipLaunchKernelGGL((layernorm_kernel<1, true>), dim3(grid), dim3(256), 0, s, a); break;
        case 4: hipLaunchKernelGGL((layernorm_kernel<2, false>), dim3(grid), dim3(256), 0, s, a); break;
        case 5: hipLaunchKernelGGL((layernorm_kernel<2, true>), dim3(grid), dim3(256), 0, s, a); break;
        case 6: hipLaunchKernelGGL((layernorm_kernel<3, false>), dim3(grid), dim3(256), 0, s, a); break;
        case 7: hipLaunchKernelGGL((layernorm_kernel<3, true>), dim3(grid), dim3(256), 0, s, a); break;
        case 8: hipLaunchKernelGGL((layernorm_kernel<4, false>), dim3(grid), dim3(256), 0, s, a); break;
        default: hipLaunchKernelGGL((layernorm_kernel<4, true>), dim3(grid), dim3(256), 0, s, a); break;
    }
    return hipGetLastError();
}

hipError_t launch_ln_reduce(const float* slabs, int nslab, const float* bias, const float* resid, const float* gamma,
                            const float* beta, float eps, int M, int D, float* xf, bf16_t* xb, hipStream_t s) {
    if (M <= 0 || D % 4 || D > 1024 || nslab < 1 || nslab > 64) return hipErrorInvalidValue;
    const int nv = (D + 255) / 256;
    const dim3 block(64 * ((nslab + 7) / 8));
    if (nv == 1) hipLaunchKernelGGL(ln_reduce_kernel<1>, dim3(M), block, 0, s, slabs, nslab, bias, resid, gamma, beta, eps, M, D, xf, xb);
    else if (nv == 2) hipLaunchKernelGGL(ln_reduce_kernel<2>, dim3(M), block, 0, s, slabs, nslab, bias, resid, gamma, beta, eps, M, D, xf, xb);
    else if (nv == 3) hipLaunchKernelGGL(ln_reduce_kernel<3>, dim3(M), block, 0, s, slabs, nslab, bias, resid, gamma, beta, eps, M, D, xf, xb);
    else hipLaunchKernelGGL(ln_reduce_kernel<4>, dim3(M), block, 0, s, slabs, nslab, bias, resid, gamma, beta, eps, M, D, xf, xb);
    return hipGetLastError();
}

hipError_t launch_pack_frags(const void* src, void* dst, int rows16, int K, int elem_bytes, hipStream_t s) {
    if (rows16 <= 0 || rows16 % 16 || K % 32 || (elem_bytes != 1 && elem_bytes != 2)) return hipErrorInvalidValue;
    const int64_t total8 = (int64_t)rows16 * K / 8;
    const dim3 grid((unsigned)((total8 + 255) / 256));
    if (elem_bytes == 2) hipLaunchKernelGGL(pack_frags_kernel<unsigned short>, grid, dim3(256), 0, s, (const unsigned short*)src, (unsigned short*)dst, K, total8);
    else hipLaunchKernelGGL(pack_frags_kernel<unsigned char>, grid, dim3(256), 0, s, (const unsigned char*)src, (unsigned char*)dst, K, total8);
    return hipGetLastError();
}

// one launch form of argmax_final_kernel: without LP the kernel is handed null sum / lp, without FORCED the empty PromptSel,
// without KEEP the empty KeepSel
template <int NV, bool LP, bool FORCED, bool KEEP>
static void argmax_final_launch(const ArgmaxArgs& a, const NextEmbed& e, const PromptSel<FORCED>& pr, const KeepSel<KEEP>& kp, hipStream_t s) {
    hipLaunchKernelGGL((argmax_final_kernel<NV, LP, FORCED, KEEP>), dim3(a.rows), dim3(256), 0, s, a.val, a.idx, a.ntiles, a.row_stride, a.row_off,
                       a.out, a.ld_out, a.sep_cnt, a.step, a.sep_id, e, LP ? a.sum : nullptr, LP ? a.lp_out : nullptr, LP ? a.ld_lp : 0, pr, kp);
}
template <bool FORCED, bool KEEP>
static void argmax_final_dispatch(const ArgmaxArgs& a, int nv, const NextEmbed& e, const PromptSel<FORCED>& pr, const KeepSel<KEEP>& kp,
                                  hipStream_t s) {
    const bool lp = a.lp_out != nullptr;
    switch (nv) {
        case 0: lp ? argmax_final_launch<0, true>(a, e, pr, kp, s) : argmax_final_launch<0, false>(a, e, pr, kp, s); break;
        case 1: lp ? argmax_final_launch<1, true>(a, e, pr, kp, s) : argmax_final_launch<1, false>(a, e, pr, kp, s); break;
        case 2: lp ? argmax_final_launch<2, true>(a, e, pr, kp, s) : argmax_final_launch<2, false>(a, e, pr, kp, s); break;
        case 3: lp ? argmax_final_launch<3, true>(a, e, pr, kp, s) : argmax_final_launch<3, false>(a, e, pr, kp, s); break;
        default: lp ? argmax_final_launch<4, true>(a, e, pr, kp, s) : argmax_final_launch<4, false>(a, e, pr, kp, s); break;
    }
}

hipError_t launch_argmax_final(const ArgmaxArgs& a, hipStream_t s) {
    const NextEmbed e = a.emb ? *a.emb : NextEmbed{};
    const int nv = a.emb ? (e.D + 255) / 256 : 0;
    if (a.emb && (nv < 1 || nv > 4 || (e.D & 3) || !e.word || !e.pos || !e.gamma || !e.beta || !e.xf || !e.xb)) return hipErrorInvalidValue;
    if ((a.sum == nullptr) != (a.lp_out == nullptr) || (a.lp_out && a.ld_lp < 1)) return hipErrorInvalidValue;
    const PromptArgs* p = a.prompt;
    if (p && (!p->ids || !p->lengths || p->max_len < 1 || p->ld < p->max_len || a.prompt_pos < 0)) return hipErrorInvalidValue;
    if (a.keep_len && (p || a.prompt_pos < 0)) return hipErrorInvalidValue;      // (the kept form is not combined with a prompt)
    if (a.keep_len)
        argmax_final_dispatch(a, nv, e, PromptSel<false>{}, KeepSel<true>{a.keep_len, a.prompt_pos}, s);
    else if (p && a.prompt_pos < p->max_len)        // (behind the longest prompt the plain forms choose the same tokens)
        argmax_final_dispatch(a, nv, e, PromptSel<true>{p->ids, p->lengths, p->ld, p->max_len, a.prompt_pos}, KeepSel<false>{}, s);
    else
        argmax_final_dispatch(a, nv, e, PromptSel<false>{}, KeepSel<false>{}, s);
    return hipGetLastError();
}

hipError_t launch_score_final(const float* amax_val, const int* amax_idx, const float* amax_sum, int ntiles, const float* tgt_logit,
                              const int64_t* ids, int ld_ids, int rows, int T, const int32_t* lengths, int64_t ignore_id, int V,
                              const ScoreOut& o, hipStream_t s) {
    if (!amax_val || !amax_idx || !amax_sum || !tgt_logit || !ids || !o.lp || ntiles <= 0 || rows <= 0 || T < 2 || ld_ids < T || V <= 0 ||
        o.ld_lp < T - 1 || (int64_t)rows * (T - 1) > 0x7fffffff)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(score_final_kernel, dim3(rows * (T - 1)), dim3(256), 0, s, amax_val, amax_idx, amax_sum, ntiles, tgt_logit, ids, ld_ids, T,
                       lengths, ignore_id, V, o.lp, o.ld_lp, o.top1_ids, o.top1_lp);
    if (o.row_sum || o.row_cnt)
        hipLaunchKernelGGL(score_rows_kernel, dim3((rows + 63) / 64), dim3(64), 0, s, (const float*)o.lp, o.ld_lp, ids, ld_ids, rows, T, lengths,
                           ignore_id, V, o.row_sum, o.row_cnt);
    return hipGetLastError();
}

hipError_t launch_distill_final(const DistillPartials& p, int ntiles, const float* t_logit, const float* s_logit, const int64_t* ids,
                                int ld_ids, int rows, int T, const int32_t* lengths, int64_t ignore_id, int V, const DistillOut& o,
                                hipStream_t s) {
    if (!p.t_max || !p.t_idx || !p.t_sum || !p.s_max || !p.s_idx || !p.s_sum || !p.cross || !o.kl || ntiles <= 0 || rows <= 0 || T < 1 ||
        V <= 0 || o.ld_kl < T || (int64_t)rows * T > 0x7fffffff)
        return hipErrorInvalidValue;
    if ((o.t_lp || o.s_lp) && (!ids || ld_ids < T || o.ld_lp < T - 1 || (o.t_lp && !t_logit) || (o.s_lp && !s_logit))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(distill_final_kernel, dim3(rows * T), dim3(256), 0, s, p, ntiles, t_logit, s_logit, ids, ld_ids, T, lengths, ignore_id,
                       V, o);
    if (o.row_kl_sum || o.row_cnt)
        hipLaunchKernelGGL(distill_rows_kernel, dim3((rows + 63) / 64), dim3(64), 0, s, (const float*)o.kl, o.ld_kl, rows, T, lengths,
                           o.row_kl_sum, o.row_cnt);
    return hipGetLastError();
}

hipError_t launch_draft_accept(const DraftAcceptArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.n < 1 || a.n > 63 || a.ld < a.n + 1 || a.ntiles <= 0 || !a.val || !a.idx || !a.ids || !a.tok || !a.ticket || !a.sep_cnt ||
        !a.host)
        return hipErrorInvalidValue;
    if ((a.sum == nullptr) != (a.lp_out == nullptr) || (a.lp_out && (!a.lp_tok || a.ld_lp < a.n))) return hipErrorInvalidValue;
    if (a.lp_out)
        hipLaunchKernelGGL(draft_accept_kernel<true>, dim3(a.B * a.n), dim3(256), 0, s, a.val, a.idx, a.ntiles, a.B, a.n, a.ids, a.ld, a.tok,
                           a.ticket, a.sep_cnt, a.sep_id, a.host, a.sum, a.lp_tok, a.lp_out, a.ld_lp);
    else
        hipLaunchKernelGGL(draft_accept_kernel<false>, dim3(a.B * a.n), dim3(256), 0, s, a.val, a.idx, a.ntiles, a.B, a.n, a.ids, a.ld, a.tok,
                           a.ticket, a.sep_cnt, a.sep_id, a.host, (const float*)nullptr, (int*)nullptr, (float*)nullptr, 0);
    return hipGetLastError();
}

hipError_t launch_draft_stage(const int64_t* draft, int ld_draft, int n, int rows, int vocab, int64_t cls, int64_t* ids, int ld, hipStream_t s) {
    if (!draft || !ids || n < 1 || rows < 1 || vocab < 1 || ld_draft < n + 1 || ld < n + 1 || (int64_t)rows * (n + 1) > 0x7fffffff)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(draft_stage_kernel, dim3((rows * (n + 1) + 255) / 256), dim3(256), 0, s, draft, ld_draft, n, rows, vocab, cls, ids, ld);
    return hipGetLastError();
}

hipError_t launch_draft_accept_rows(const DraftAcceptRowsArgs& a, hipStream_t s) {
    if (a.B <= 0 || a.n < 1 || a.n > 63 || (int64_t)a.B * a.n > 0x7fffffff || a.ld < a.n + 1 || a.ntiles <= 0 || !a.val || !a.idx || !a.ids ||
        !a.len || !a.tok || !a.row_res || !a.ticket || !a.sep_cnt || !a.host)
        return hipErrorInvalidValue;
    if ((a.sum == nullptr) != (a.lp_out == nullptr) || (a.lp_out && (!a.lp_tok || a.ld_lp < a.n))) return hipErrorInvalidValue;
    if (a.lp_out)
        hipLaunchKernelGGL(draft_accept_rows_kernel<true>, dim3(a.B * a.n), dim3(256), 0, s, a.val, a.idx, a.ntiles, a.B, a.n, a.ids, a.ld, a.len,
                           a.tok, a.row_res, a.ticket, a.sep_cnt, a.sep_id, a.host, a.host_rows, a.sum, a.lp_tok, a.lp_out, a.ld_lp);
    else
        hipLaunchKernelGGL(draft_accept_rows_kernel<false>, dim3(a.B * a.n), dim3(256), 0, s, a.val, a.idx, a.ntiles, a.B, a.n, a.ids, a.ld, a.len,
                           a.tok, a.row_res, a.ticket, a.sep_cnt, a.sep_id, a.host, a.host_rows, (const float*)nullptr, (int*)nullptr,
                           (float*)nullptr, 0);
    return hipGetLastError();
}

size_t beam_topk_scratch_bytes(int B, int beams, int V, int K) {
    const size_t n = (size_t)B * beams * ((V + BT_CHUNK - 1) / BT_CHUNK);
    return n * 8 + n * K * 8;                          // chunk (max, sum) + K (value, index) candidates per chunk
}

template <int KMAX>
static void beam_topk_launch(const CandArgs& c, int K, int nch, void* scratch, hipStream_t s) {
    const size_t n = (size_t)c.B * c.beams * nch;
    float2* stats = (float2*)scratch;
    float* cval = (float*)(stats + n);
    int* cidx = (int*)(cval + n * K);
    const BeamPenalty<true> pen{c.prefix_ids, c.ld_ids, c.cur_len, c.rp};
    if (c.bn && c.rp != 1.0f)
        hipLaunchKernelGGL((beam_topk_chunks_kernel<KMAX, true, true>), dim3((unsigned)n), dim3(256), 0, s, c.logits, c.ld, c.V, K, nch, stats, cval,
                           cidx, pen, BeamBan<true>{c.bn->mask, c.bn->ld});
    else if (c.bn)
        hipLaunchKernelGGL((beam_topk_chunks_kernel<KMAX, false, true>), dim3((unsigned)n), dim3(256), 0, s, c.logits, c.ld, c.V, K, nch, stats, cval,
                           cidx, BeamPenalty<false>{}, BeamBan<true>{c.bn->mask, c.bn->ld});
    else if (c.rp != 1.0f)
        hipLaunchKernelGGL((beam_topk_chunks_kernel<KMAX, true>), dim3((unsigned)n), dim3(256), 0, s, c.logits, c.ld, c.V, K, nch, stats, cval, cidx,
                           pen, BeamBan<false>{});
    else
        hipLaunchKernelGGL((beam_topk_chunks_kernel<KMAX, false>), dim3((unsigned)n), dim3(256), 0, s, c.logits, c.ld, c.V, K, nch, stats, cval, cidx,
                           BeamPenalty<false>{}, BeamBan<false>{});
    hipLaunchKernelGGL(beam_topk_merge_kernel<KMAX>, dim3(c.B), dim3(64), 0, s, stats, cval, cidx, c.beam_scores, c.beams, c.V, K, nch, c.out_scores,
                       c.out_idx);
}

// what launch_beam_topk and launch_sample_rows check alike: the penalty's prefix (rp == 1: neither checked nor read) and the ban mask
static bool cand_args_ok(const CandArgs& c) {
    if (c.rp != 1.0f && (!c.prefix_ids || c.cur_len < 1 || c.ld_ids < c.cur_len || !(c.rp > 0.f) || !std::isfinite(c.rp))) return false;
    return !c.bn || (c.bn->mask && c.bn->ld >= (c.V + 15) / 16);
}

hipError_t launch_beam_topk(const CandArgs& c, int K, void* scratch, hipStream_t s) {
    const int nch = (c.V + BT_CHUNK - 1) / BT_CHUNK;
    if (c.B <= 0 || c.beams <= 0 || c.beams > 16 || K <= 0 || K > 16 || K > c.beams * c.V || nch > 64 || !scratch) return hipErrorInvalidValue;
    if (!cand_args_ok(c)) return hipErrorInvalidValue;
    if (K <= 8) beam_topk_launch<8>(c, K, nch, scratch, s);
    else beam_topk_launch<16>(c, K, nch, scratch, s);
    return hipGetLastError();
}

template <bool BAN>
static hipError_t sample_rows_launch(const CandArgs& c, int pn, const SampleOpt& o, const SampleStats& st, const BeamBan<BAN>& ban, hipStream_t s) {
    if (const hipError_t e = set_dynamic_lds_once<sample_rows_kernel<BAN>>(SR_MAX_V * 4); e != hipSuccess) return e;
    hipLaunchKernelGGL(sample_rows_kernel<BAN>, dim3(c.B * c.beams), dim3(SR_THREADS), (size_t)c.V * 4, s, c.logits, c.ld, c.V, c.beam_scores,
                       c.prefix_ids, c.ld_ids, c.cur_len, c.rp, c.beams, pn, o.temperature, o.top_k, o.top_p, (unsigned)o.seed,
                       (unsigned)(o.seed >> 32), c.out_scores, c.out_idx, st.kept_out, st.logz_out, ban);
    return hipGetLastError();
}

hipError_t launch_sample_rows(const CandArgs& c, int pn, const SampleOpt& o, const SampleStats& st, hipStream_t s) {
    if (c.B <= 0 || c.beams <= 0 || c.beams > 16 || pn <= 0 || c.beams * pn > 16 || pn > c.V || c.V > SR_MAX_V || c.ld < c.V || c.cur_len < 0)
        return hipErrorInvalidValue;
    if (!(o.temperature > 0.f) || !std::isfinite(o.temperature) || o.top_k < 0 || !(o.top_p > 0.f) || !(o.top_p <= 1.f)) return hipErrorInvalidValue;
    if (!cand_args_ok(c)) return hipErrorInvalidValue;
    return c.bn ? sample_rows_launch(c, pn, o, st, BeamBan<true>{c.bn->mask, c.bn->ld}, s) : sample_rows_launch(c, pn, o, st, BeamBan<false>{}, s);
}

hipError_t launch_ban_mask(const int64_t* ids, int ld_ids, int rows, int cur_len, int n, int min_length, int sep_id,
                           const int32_t* suppress, int n_suppress, int V, uint16_t* mask, int ld_mask, hipStream_t s) {
    if (!ids || !mask || rows <= 0 || cur_len < 0 || ld_ids < cur_len || n < 0 || min_length < 0 || n_suppress < 0 || n_suppress > 256 ||
        (n_suppress > 0 && !suppress) || V <= 0 || V > BM_MAX_V || ld_mask < (V + 15) / 16 || (ld_mask & 1) || ((uintptr_t)mask & 3))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(ban_mask_kernel, dim3(rows), dim3(256), 0, s, ids, ld_ids, cur_len, n, min_length, sep_id, suppress, n_suppress, V,
                       (unsigned*)mask, ld_mask / 2);
    return hipGetLastError();
}

static BeamState beam_state(const BeamBuffers& bb) {
    return BeamState{{bb.ids0, bb.ids1}, bb.beam_scores, bb.words, bb.src_rows, bb.done, bb.hyp_len, bb.hyp_score, bb.hyp_ids};
}

hipError_t launch_beam_init(const BeamBuffers& bb, int B, int beams, int n, int max_len, int cls, hipStream_t s) {
    if (n < 1 || n > 16) return hipErrorInvalidValue;
    hipLaunchKernelGGL(beam_init_kernel, dim3((B * std::max(beams, n) + 63) / 64), dim3(64), 0, s, beam_state(bb), B, beams, n, max_len, cls);
    return hipGetLastError();
}

// the three kernels of a step, with or without a prompt: draws, one hypothesis slot, n slots
template <bool FORCED>
static void beam_step_launch(const BeamBuffers& bb, const BeamStepArgs& a, const PromptSel<FORCED>& pr, hipStream_t s) {
    if (a.sampled)
        hipLaunchKernelGGL((beam_step_nbest_kernel<true, FORCED>), dim3(a.B), dim3(64), 0, s, beam_state(bb), a.n, a.cand_scores, a.cand_idx, a.beams,
                           a.K, a.V, a.cur_len, a.max_len, a.eos, a.length_penalty, a.cur, pr);
    else if (a.n == 1)
        hipLaunchKernelGGL(beam_step_kernel<FORCED>, dim3(a.B), dim3(64), 0, s, beam_state(bb), a.cand_scores, a.cand_idx, a.beams, a.K, a.V,
                           a.cur_len, a.max_len, a.eos, a.length_penalty, a.cur, pr);
    else
        hipLaunchKernelGGL((beam_step_nbest_kernel<false, FORCED>), dim3(a.B), dim3(64), 0, s, beam_state(bb), a.n, a.cand_scores, a.cand_idx, a.beams,
                           a.K, a.V, a.cur_len, a.max_len, a.eos, a.length_penalty, a.cur, pr);
}

hipError_t launch_beam_step(const BeamBuffers& bb, const BeamStepArgs& a, hipStream_t s) {
    if (a.beams > 16 || a.K > 16 || a.n < 1 || a.n > 16) return hipErrorInvalidValue;
    const PromptArgs* p = a.prompt;
    if (p && (!p->ids || !p->lengths || p->max_len < 1 || p->ld < p->max_len || p->max_len >= a.max_len)) return hipErrorInvalidValue;
    if (p && a.cur_len < p->max_len)                // (behind the longest prompt no clip is forced: the plain forms)
        beam_step_launch(bb, a, PromptSel<true>{p->ids, p->lengths, p->ld, p->max_len, a.cur_len}, s);
    else
        beam_step_launch(bb, a, PromptSel<false>{}, s);
    return hipGetLastError();
}

hipError_t launch_beam_finish(const BeamBuffers& bb, int n, int B, int max_len, int eos, const BeamFinishOut& o, hipStream_t s) {
    if (n < 1 || n > 16) return hipErrorInvalidValue;
    hipLaunchKernelGGL(beam_finish_kernel, dim3(B, n), dim3(64), 0, s, beam_state(bb), n, max_len, eos, o.decoded, o.logprobs, o.first_decoded,
                       o.first_logprobs);
    return hipGetLastError();
}

hipError_t launch_im2col(const float* frames, bf16_t* patches, int nf, int img, int p, int Kp, hipStream_t s) {
    const int G = img / p;
    if (p % 4 == 0 && img % 4 == 0) {
        const int64_t total = (int64_t)nf * G * G * (Kp / 4);
        hipLaunchKernelGGL(im2col_kernel<4>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, frames, patches, nf, img, p, Kp);
    } else if (p % 2 == 0) {
        const int64_t total = (int64_t)nf * G * G * (Kp / 2);
        hipLaunchKernelGGL(im2col_kernel<2>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, frames, patches, nf, img, p, Kp);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}



// ---- V of the image prefix as OCP e4m3 codes + one power-of-two scale per (token, head) (opt-in kv_cache = v_e4m3) -------
// kv: [rows][3D] bf16 (q | k | v of one decoder layer's image rows) -> v8 [H][pitch][64] codes, vs [H][pitch] scales, HEAD-MAJOR: the
// V stream of one (row, head) unit of txt_block is one contiguous run of 64-byte records (two keys per cache line).  Eight lanes per
// (row, head): 8 values each; scale = the smallest 2^e, e >= -126, with amax <= 448 * 2^e (exact: for amax >= 2^-118,
// amax / 2^(E-8) lies in [256, 512) and is compared with 448 after an exact scaling; a smaller amax keeps the floor 2^-126 and small
// codes; an all-zero group has scale 1), codes round to nearest even; code * scale is a bf16 value.
namespace {
__global__ __launch_bounds__(256) void kv_quant_v_kernel(const bf16_t* __restrict__ kv, unsigned char* __restrict__ v8, float* __restrict__ vs,
                                                         int64_t groups, int D, int H, int64_t pitch) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t gi = t >> 3;
    const int sub = (int)(t & 7);
    const bool live = gi < groups;
    const int64_t g = live ? gi : groups - 1;
    const int64_t row = g / H;
    const int head = (int)(g - row * H);
    const bf16x8 x = *(const bf16x8*)(kv + row * 3 * D + 2 * D + head * 64 + sub * 8);
    float f[8], amax = 0.f;
#pragma unroll
    for (int d = 0; d < 8; ++d) { f[d] = bf2f((bf16_t)x[d]); amax = fmaxf(amax, fabsf(f[d])); }
    amax = fmaxf(amax, __shfl_xor(amax, 1));
    amax = fmaxf(amax, __shfl_xor(amax, 2));
    amax = fmaxf(amax, __shfl_xor(amax, 4));
    float scale = 1.0f;
    if (amax > 0.f) {
        const int E = (int)((__float_as_uint(amax) >> 23) & 0xff) - 127;          // floor(log2 amax); -127 for a denormal amax
        // amax / scale in [256, 512); never below 2^-126: for amax < 2^-118 the exponent field E - 8 + 127 would be <= 0, i.e. a
        // scale of 0, -inf or worse (and 0 * inf = NaN in txt_block) -- such a group keeps the smallest normal scale, its codes are small
        scale = __uint_as_float((unsigned)((E - 8 < -126 ? -126 : E - 8) + 127) << 23);
        if (amax > 448.0f * scale) scale *= 2.0f;
    }
    const float inv = 1.0f / scale;                                                // a power of two: exact
    uint2 q;
    q.x = pack_fp8x4(f[0] * inv, f[1] * inv, f[2] * inv, f[3] * inv);
    q.y = pack_fp8x4(f[4] * inv, f[5] * inv, f[6] * inv, f[7] * inv);
    if (live) {
        *(uint2*)(v8 + ((int64_t)head * pitch + row) * 64 + sub * 8) = q;
        if (sub == 0) vs[(int64_t)head * pitch + row] = scale;
    }
}
}  // namespace

hipError_t launch_kv_quant_v(const bf16_t* kv, unsigned char* v8, float* vs, int rows, int D, int H, int64_t pitch, hipStream_t s) {
    if (rows <= 0 || H * 64 != D || pitch < rows) return hipErrorInvalidValue;
    const int64_t groups = (int64_t)rows * H;
    hipLaunchKernelGGL(kv_quant_v_kernel, dim3((unsigned)((groups * 8 + 255) / 256)), dim3(256), 0, s, kv, v8, vs, groups, D, H, pitch);
    return hipGetLastError();
}

hipError_t launch_cast_bf16(const float* in, bf16_t* out, int64_t n, hipStream_t s) {
    if (n % 4) return hipErrorInvalidValue;
    const int64_t n4 = n / 4;
    hipLaunchKernelGGL(cast_bf16_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, in, out, n4);
    return hipGetLastError();
}

hipError_t launch_gather_hidden(const float* img, const float* txt, float* out, int n_entries, int B, int S_img, int T, int D,
                                size_t img_entry_stride, size_t txt_entry_stride, hipStream_t s) {
    if (B <= 0 || n_entries <= 0 || S_img <= 0 || T <= 0 || D % 4) return hipErrorInvalidValue;
    const size_t rows = (size_t)B * n_entries * (S_img + T);
    hipLaunchKernelGGL(gather_hidden_kernel, dim3((unsigned)rows), dim3(256), 0, s, img, txt, out, n_entries, S_img, T, D,
                       img_entry_stride, txt_entry_stride);
    return hipGetLastError();
}

hipError_t launch_window_scatter(const float* src, float* ring, int B, int n, int F, int head, int rows_per_frame, int D, hipStream_t s) {
    if (B <= 0 || n <= 0 || n > F || head < 0 || head >= F || rows_per_frame <= 0 || D % 4) return hipErrorInvalidValue;
    const int64_t frame4 = (int64_t)rows_per_frame * D / 4;
    const unsigned gx = (unsigned)std::min<int64_t>((frame4 + 255) / 256, 64);
    hipLaunchKernelGGL(window_scatter_kernel, dim3(gx, (unsigned)(B * n)), dim3(256), 0, s, src, ring, n, F, head, frame4);
    return hipGetLastError();
}

hipError_t launch_window_assemble(const float* ring, const float* temporal, bf16_t* out, float* vis, int B, int F, int head, int N, int D,
                                  hipStream_t s) {
    if (B <= 0 || F <= 0 || head < 0 || head >= F || N <= 0 || D % 4 || D > 1024) return hipErrorInvalidValue;
    const int rows = B * F * N;
    hipLaunchKernelGGL(window_assemble_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, ring, temporal, out, vis, rows, F,
                       head, N, D);
    return hipGetLastError();
}

hipError_t launch_ragged_tables(const RaggedCounts& rc, int N, int32_t* off, int32_t* len, int32_t* pos, hipStream_t s) {
    if (rc.B <= 0 || rc.B > 256 || N <= 0 || !off || !len || !pos) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ragged_tables_kernel, dim3(1), dim3(64), 0, s, rc, N, off, len, pos);
    return hipGetLastError();
}

hipError_t launch_ragged_temporal(const float* ln, const float* temporal, const int32_t* pos, bf16_t* out, float* vis, int frames, int N,
                                  int D, hipStream_t s) {
    if (frames <= 0 || N <= 0 || D % 4 || D > 1024 || !ln || !temporal || !pos || !out) return hipErrorInvalidValue;
    const int rows = frames * N;
    hipLaunchKernelGGL(ragged_temporal_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, ln, temporal, pos, out, vis, rows, N, D);
    return hipGetLastError();
}

hipError_t launch_dequant_fp8_batch(const DequantBatch& b, hipStream_t s) {
    if (b.n <= 0 || b.n > 4) return hipErrorInvalidValue;
    int64_t mx = 0;
    for (int i = 0; i < b.n; ++i) {
        if ((b.K[i] & 15) || !b.w8[i] || !b.scale[i] || !b.out[i]) return hipErrorInvalidValue;
        mx = std::max(mx, b.n16[i]);
    }
    hipLaunchKernelGGL(dequant_fp8_batch_kernel, dim3((unsigned)((mx + 255) / 256), (unsigned)b.n), dim3(256), 0, s, b);
    return hipGetLastError();
}

hipError_t launch_dequant_fp8(const unsigned char* w8, const float* scale, bf16_t* out, int rows, int K, hipStream_t s) {
    if (rows <= 0 || K <= 0 || K % 16) return hipErrorInvalidValue;
    const int64_t n16 = (int64_t)rows * K / 16;
    hipLaunchKernelGGL(dequant_fp8_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, s, w8, scale, out, K, n16);
    return hipGetLastError();
}

hipError_t launch_embed_text(const int64_t* ids, int ld_ids, int rows, int T, int t0, const float* word,
                             const float* pos, const float* gamma, const float* beta, float eps, int D, int vocab,
                             float* x_f32, bf16_t* x_bf16, hipStream_t s) {
    const int grid = (rows * T + 3) / 4;
    const int nv = (D + 255) / 256;
    if (nv == 1) hipLaunchKernelGGL(embed_text_kernel<1>, dim3(grid), dim3(256), 0, s, ids, ld_ids, rows, T, t0, word, pos, gamma, beta, eps, D, vocab, x_f32, x_bf16);
    else if (nv == 2) hipLaunchKernelGGL(embed_text_kernel<2>, dim3(grid), dim3(256), 0, s, ids, ld_ids, rows, T, t0, word, pos, gamma, beta, eps, D, vocab, x_f32, x_bf16);
    else if (nv == 3) hipLaunchKernelGGL(embed_text_kernel<3>, dim3(grid), dim3(256), 0, s, ids, ld_ids, rows, T, t0, word, pos, gamma, beta, eps, D, vocab, x_f32, x_bf16);
    else hipLaunchKernelGGL(embed_text_kernel<4>, dim3(grid), dim3(256), 0, s, ids, ld_ids, rows, T, t0, word, pos, gamma, beta, eps, D, vocab, x_f32, x_bf16);
    return hipGetLastError();
}

hipError_t launch_finish_steps(const int32_t* sep_cnt, int rows, int max_len, int stop, int32_t* steps_out, hipStream_t s) {
    hipLaunchKernelGGL(finish_steps_kernel, dim3(1), dim3(1), 0, s, sep_cnt, rows, max_len, stop, steps_out);
    return hipGetLastError();
}

hipError_t launch_fill_prompt(int64_t* p, int ld, int rows, const PromptArgs& prompt, hipStream_t s) {
    if (!p || !prompt.ids || !prompt.lengths || rows < 1 || prompt.max_len < 1 || prompt.ld < prompt.max_len || ld < prompt.max_len)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(fill_prompt_kernel, dim3((rows * prompt.max_len + 63) / 64), dim3(64), 0, s, p, ld, rows, prompt.ids, prompt.ld,
                       prompt.lengths, prompt.max_len);
    return hipGetLastError();
}

hipError_t launch_fill_i64(int64_t* p, int ld, int rows, int64_t v, hipStream_t s) {
    hipLaunchKernelGGL(fill_i64_kernel, dim3((rows + 63) / 64), dim3(64), 0, s, p, ld, rows, v);
    return hipGetLastError();
}

hipError_t launch_gather_txt_rows(const bf16_t* src, bf16_t* dst, const int32_t* src_rows, int rows,
                                  int t_len, int Tmax, int width, int layers, size_t layer_stride, hipStream_t s) {
    if (rows <= 0 || layers <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_txt_rows_kernel, dim3(rows, layers), dim3(256), 0, s, src, dst, src_rows, t_len, Tmax, width, layer_stride);
    return hipGetLastError();
}
