// HBM-bound row kernels of the image path and of the weights: LayerNorm (one wave per row, 16-byte vector loads), patch gather
// (im2col of NCHW fp32 frames, coalesced 16-B reads along W), and the copies, casts and quantisers around them.  The text rows'
// kernels (embedding, split-K reduce, token selection) are select.hip, candidate generation and the beam state search.hip.
// Topic by topic: the kernels, then their launchers.
#include "kernels.h"
#include <algorithm>
#include "ln_canon.h"

// ---- LayerNorm -------------------------------------------------------------------------------
// One wave per row; lane holds NV float4 at columns 256*i + 4*lane (1 KiB contiguous per wave-instruction), fp32
// throughout.  CANON (D a multiple of 64): the segmented statistics of ln_canon.h -- 16 lanes x 4 columns are one
// 64-column segment, so (i, lane >> 4) names segment 4 i + (lane >> 4) -- bit for bit what the GEMM epilogue that
// normalises its own rows computes.  Otherwise: two-pass (mean, then centred variance) over the wave.
namespace {
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

// ---- im2col ----------------------------------------------------------------------------------
// thread = 4 consecutive px of one (patch row, c, py): one 16-B fp32 read, one 8-B bf16 write.
// p % 4 == 0 fast path; generic path handles p = 14 (ViT-L/14) with 2-element pieces.
namespace {
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
}  // namespace
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

namespace {
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

hipError_t launch_gather_txt_rows(const bf16_t* src, bf16_t* dst, const int32_t* src_rows, int rows,
                                  int t_len, int Tmax, int width, int layers, size_t layer_stride, hipStream_t s) {
    if (rows <= 0 || layers <= 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_txt_rows_kernel, dim3(rows, layers), dim3(256), 0, s, src, dst, src_rows, t_len, Tmax, width, layer_stride);
    return hipGetLastError();
}

// ---- frame window (gitcap_window_*) ----------------------------------------------------------
// push: the ln_post rows of B x n new frames ([B][n][rows_per_frame][D], contiguous) -> ring slots (head + j) % F of their
// clip ([B][F][rows_per_frame][D]).  A plain copy, 16 B per lane; blockIdx.y = frame (b, j).
namespace {
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
}  // namespace
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

// ---- ragged batches (gitcap_attach_frame_counts) ------------------------------------------------
// The tables of a packed batch from its per-clip frame counts (by value: at most 256 clips).  One thread: a few hundred adds.
namespace {
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
}  // namespace
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

// ---- stream pool (gitcap_pool_*) -----------------------------------------------------------------
// The window kernels with the frame's ring slot read from a table the host planned (host_logic.h: pool_plan), so streams at
// different fill levels and ring positions share one launch.  Both: one wave per row, lane = 4 consecutive columns (16-byte reads
// and writes of consecutive lanes), grid = rows / 4; every destination row has one writer.
namespace {
// push: row (i, tok) of the packed staging rows [frames][N][D] -> ring frame dst[i], a plain copy
__global__ __launch_bounds__(256) void pool_scatter_kernel(const float* __restrict__ stage, float* __restrict__ ring,
                                                           const int32_t* __restrict__ dst, int rows, int N, int D) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* s = stage + (size_t)row * D;
    float* d = ring + ((size_t)dst[row / N] * N + row % N) * D;
    for (int c = lane * 4; c < D; c += 256) *(f32x4*)(d + c) = *(const f32x4*)(s + c);
}

// caption: row (g, tok) of the decoder input = bf16(ring[src[g]][tok] + temporal[pos[g]]): ragged_temporal_kernel's lone fp32 add
// (no contraction) and pack_bf2, i.e. the fused ln_post epilogue's bits; temporal == nullptr (a model without the table): no add
__global__ __launch_bounds__(256) void pool_assemble_kernel(const float* __restrict__ ring, const float* __restrict__ temporal,
                                                            const int32_t* __restrict__ src, const int32_t* __restrict__ pos,
                                                            bf16_t* __restrict__ out, int rows, int N, int D) {
    const int lane = threadIdx.x & 63;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int g = row / N;
    const float* x = ring + ((size_t)src[g] * N + row % N) * D;
    const float* t = temporal ? temporal + (size_t)pos[g] * D : nullptr;
    for (int c = lane * 4; c < D; c += 256) {
        f32x4 y = *(const f32x4*)(x + c);
        if (t) y += *(const f32x4*)(t + c);
        uint2 o;
        o.x = pack_bf2(y[0], y[1]);
        o.y = pack_bf2(y[2], y[3]);
        *(uint2*)(out + (size_t)row * D + c) = o;
    }
}
}  // namespace
hipError_t launch_pool_scatter(const PoolScatterArgs& a, hipStream_t s) {
    if (!a.stage || !a.ring || !a.dst || a.frames <= 0 || a.N <= 0 || a.D <= 0 || a.D % 4 || (int64_t)a.frames * a.N > 0x7fffffff)
        return hipErrorInvalidValue;
    const int rows = a.frames * a.N;
    hipLaunchKernelGGL(pool_scatter_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, a.stage, a.ring, a.dst, rows, a.N, a.D);
    return hipGetLastError();
}

hipError_t launch_pool_assemble(const PoolAssembleArgs& a, hipStream_t s) {
    if (!a.ring || !a.src || !a.out || (a.temporal && !a.pos) || a.frames <= 0 || a.N <= 0 || a.D <= 0 || a.D % 4 || a.D > 1024 ||
        (int64_t)a.frames * a.N > 0x7fffffff)
        return hipErrorInvalidValue;
    const int rows = a.frames * a.N;
    hipLaunchKernelGGL(pool_assemble_kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, a.ring, a.temporal, a.src, a.pos, a.out,
                       rows, a.N, a.D);
    return hipGetLastError();
}

// e4m3 weight panel -> bf16 staging panel for the big-tile GEMMs (16 values per thread: 16-B read, 32-B write)
namespace {
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
}  // namespace
hipError_t launch_dequant_fp8(const unsigned char* w8, const float* scale, bf16_t* out, int rows, int K, hipStream_t s) {
    if (rows <= 0 || K <= 0 || K % 16) return hipErrorInvalidValue;
    const int64_t n16 = (int64_t)rows * K / 16;
    hipLaunchKernelGGL(dequant_fp8_kernel, dim3((unsigned)((n16 + 255) / 256)), dim3(256), 0, s, w8, scale, out, K, n16);
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

// ---- fragment-major copy of a GEMM weight for the weight-streaming text kernels ------------------------------------------
// src [Npad16][K] (ESZ-byte elements: bf16, or e4m3 codes) -> dst [tile = n / 16][k32 = k / 32][lane][8 elements] with
// lane = n % 16 + 16 * ((k % 32) / 8): the MFMA operand a lane of skinny.hip / txtblock.hip / ffn_txt.hip loads for k-step
// k32 of tile n / 16 is 16 (8) contiguous bytes, a wave instruction reads 1 KiB (512 B) contiguous and a tile's fragments
// are one contiguous run.  Measured (tools/probe/pull_probe.hip): a CU pulls 48 KiB per wave at 47 GB/s in the row-major
// pattern (16 segments of 64 B per instruction) and at 170 GB/s (71 from cold caches) from this layout.
namespace {
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
}  // namespace
hipError_t launch_pack_frags(const void* src, void* dst, int rows16, int K, int elem_bytes, hipStream_t s) {
    if (rows16 <= 0 || rows16 % 16 || K % 32 || (elem_bytes != 1 && elem_bytes != 2)) return hipErrorInvalidValue;
    const int64_t total8 = (int64_t)rows16 * K / 8;
    const dim3 grid((unsigned)((total8 + 255) / 256));
    if (elem_bytes == 2) hipLaunchKernelGGL(pack_frags_kernel<unsigned short>, grid, dim3(256), 0, s, (const unsigned short*)src, (unsigned short*)dst, K, total8);
    else hipLaunchKernelGGL(pack_frags_kernel<unsigned char>, grid, dim3(256), 0, s, (const unsigned char*)src, (unsigned char*)dst, K, total8);
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
