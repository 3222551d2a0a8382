// TinyViT image encoder of the student captioner (SURVEY.md par. 8 row f.2): timm's TinyVit as the reference loads it
// with features_only=True (src/models/model.py:35-47, :108-126), behind the C ABI declared in include/gitcap.h
// ("student image encoder" section).  DESIGN.md "TinyViT encoder" lists the bf16 rounding points and the parts of the
// architecture that are written from the published description and not checked against timm.
//
// Activations are bf16 NHWC rows [n*H*W][C]; every layer accumulates in fp32 and rounds its output once, to bf16.
//   tv_gemm     one wave = a 32(m) x 32(n) output tile, v_mfma_f32_16x16x32_bf16, operands read as 16-B vectors straight
//               from global memory (the weight panel of a launch is a few hundred KB and stays in L2).  One-wave
//               workgroups: a single clip's stage-3 launch (294 rows) still spreads over 10 x N/32 CUs.  Fused epilogues:
//               +bias (the folded BatchNorm), GELU, +residual, GELU after the residual (MBConv act3).  Serves the 1x1
//               convs, the Linears and the two stem convs (after tv_im2col).
//   tv_dwconv   depthwise 3x3 (stride 1 or 2) + folded BN (+ GELU), one thread = 8 channels of one output pixel.
//   tv_ln       LayerNorm, one wave per row, two-pass fp32 statistics.
//   tv_attn     windowed attention with the relative-position bias table: one workgroup = one (window, head), one thread
//               per query, K / V of the window in LDS (fp32), online softmax in fp32; window partition and reverse are
//               index math on the NHWC rows.
//   tv_pool     mean of the stage-3 map over H*W -> fp32 memory, ascending pixel order.
//   tv_to_nchw  bf16 NHWC rows -> fp32 NCHW feature map (only when the caller asks for feature maps).
// gitcap_tinyvit_encode_raw takes uint8 camera frames: the first stem convolution's im2col rows then come from
// preprocess_stem_kernel (preproc.hip: the frame transform fused with that gather) and everything behind them is shared.
// No atomics: every output element is summed in an order fixed by its own row, so results do not depend on the batch.
#include "../../include/gitcap.h"
#include "kernels.h"
#include "host_util.h"

#include <cmath>
#include <map>
#include <string>
#include <vector>

namespace {

enum { TV_GELU = 1, TV_RES = 2, TV_RES_GELU = 4 };

struct TvGemmArgs {
    const bf16_t* A; int lda;        // [M][K] activations
    const bf16_t* W;                 // [N][K] weight (K contiguous)
    const float* bias;               // [N]
    const bf16_t* res; int ldr;      // [M][N] residual (TV_RES)
    bf16_t* out; int ldo;            // [M][N]
    int M, N, K;
};

// out = epi(A . W^T + bias).  Lane l of a 16x16x32 MFMA holds 8 consecutive k of row (l & 15) for both operands and
// 4 consecutive n (4 * (l >> 4) + r) of row m = l & 15 of the accumulator (the map of gemm.hip).  Rows >= M and weight rows
// >= N are clamped for the loads and skipped by the stores; N % 4 == 0 so a lane's 4 columns are all valid or all not.
template <int EPI>
__global__ __launch_bounds__(64) void tv_gemm_kernel(TvGemmArgs a) {
    const int lane = threadIdx.x, frow = lane & 15, fq = lane >> 4;
    const int m0 = blockIdx.x * 32, n0 = blockIdx.y * 32;
    const bf16_t* ap[2];
    const bf16_t* wp[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) ap[j] = a.A + (size_t)min(m0 + 16 * j + frow, a.M - 1) * a.lda + 8 * fq;
#pragma unroll
    for (int i = 0; i < 2; ++i) wp[i] = a.W + (size_t)min(n0 + 16 * i + frow, a.N - 1) * a.K + 8 * fq;
    f32x4 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x8 af[2], wf[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) af[j] = *(const bf16x8*)ap[j];
#pragma unroll
    for (int i = 0; i < 2; ++i) wf[i] = *(const bf16x8*)wp[i];
    for (int k = 32; k <= a.K; k += 32) {
        bf16x8 an[2], wn[2];
        if (k < a.K) {          // next k-step requested before this one's MFMAs
#pragma unroll
            for (int j = 0; j < 2; ++j) an[j] = *(const bf16x8*)(ap[j] + k);
#pragma unroll
            for (int i = 0; i < 2; ++i) wn[i] = *(const bf16x8*)(wp[i] + k);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[i], af[j], acc[i][j], 0, 0, 0);
        if (k < a.K) {
#pragma unroll
            for (int j = 0; j < 2; ++j) af[j] = an[j];
#pragma unroll
            for (int i = 0; i < 2; ++i) wf[i] = wn[i];
        }
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int n = n0 + 16 * i + 4 * fq;
        if (n >= a.N) continue;
        const f32x4 b4 = *(const f32x4*)(a.bias + n);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int m = m0 + 16 * j + frow;
            if (m >= a.M) continue;
            f32x4 v = acc[i][j] + b4;
            if (EPI & TV_GELU) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = erf_gelu(v[r]);
            }
            if (EPI & TV_RES) {
                const uint2 rr = *(const uint2*)(a.res + (size_t)m * a.ldr + n);
                v[0] += bf2f((bf16_t)(rr.x & 0xffff)); v[1] += bf2f((bf16_t)(rr.x >> 16));
                v[2] += bf2f((bf16_t)(rr.y & 0xffff)); v[3] += bf2f((bf16_t)(rr.y >> 16));
            }
            if (EPI & TV_RES_GELU) {
#pragma unroll
                for (int r = 0; r < 4; ++r) v[r] = erf_gelu(v[r]);
            }
            uint2 o;
            o.x = pack_bf2(v[0], v[1]);
            o.y = pack_bf2(v[2], v[3]);
            *(uint2*)(a.out + (size_t)m * a.ldo + n) = o;
        }
    }
}

// 3x3 stride-2 pad-1 patches of the stem convs: out[m][k] (m = (frame, oy, ox), k = ci * 9 + ky * 3 + kx, the flattening
// of a torch conv weight [Cout][Cin][3][3]; zero for k >= Cin * 9).  F32_NCHW: the normalised frames; else bf16 NHWC rows.
template <bool F32_NCHW>
__global__ __launch_bounds__(256) void tv_im2col_kernel(const void* __restrict__ in, bf16_t* __restrict__ out, int n, int H, int W,
                                                        int Cin, int Ho, int Wo, int Kp) {
    const int64_t total = (int64_t)n * Ho * Wo * Kp;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int k = (int)(e % Kp);
        const int64_t m = e / Kp;
        const int ox = (int)(m % Wo), oy = (int)((m / Wo) % Ho), f = (int)(m / ((int64_t)Wo * Ho));
        float v = 0.f;
        if (k < Cin * 9) {
            const int ci = k / 9, t = k % 9, iy = 2 * oy - 1 + t / 3, ix = 2 * ox - 1 + t % 3;
            if (iy >= 0 && iy < H && ix >= 0 && ix < W) {
                if (F32_NCHW) v = ((const float*)in)[(((size_t)f * Cin + ci) * H + iy) * W + ix];
                else v = bf2f(((const bf16_t*)in)[(((size_t)f * H + iy) * W + ix) * Cin + ci]);
            }
        }
        out[e] = f2bf(v);
    }
}

// depthwise 3x3, pad 1, stride S: out[f][oy][ox][c] = sum_taps x * w[tap][c] (taps in ky, kx order) + bias[c] (-> GELU)
template <bool GELU>
__global__ __launch_bounds__(256) void tv_dwconv_kernel(const bf16_t* __restrict__ x, const float* __restrict__ w9,
                                                        const float* __restrict__ bias, bf16_t* __restrict__ out, int n, int H,
                                                        int W, int C, int stride, int Ho, int Wo) {
    const int C8 = C / 8;
    const int64_t total = (int64_t)n * Ho * Wo * C8;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int c = (int)(e % C8) * 8;
        const int64_t m = e / C8;
        const int ox = (int)(m % Wo), oy = (int)((m / Wo) % Ho), f = (int)(m / ((int64_t)Wo * Ho));
        float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < 9; ++t) {
            const int iy = stride * oy - 1 + t / 3, ix = stride * ox - 1 + t % 3;
            if (iy < 0 || iy >= H || ix < 0 || ix >= W) continue;
            const bf16x8 xv = *(const bf16x8*)(x + (((size_t)f * H + iy) * W + ix) * C + c);
            const f32x4 w0 = *(const f32x4*)(w9 + (size_t)t * C + c), w1 = *(const f32x4*)(w9 + (size_t)t * C + c + 4);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                acc[r] += bf2f((bf16_t)xv[r]) * w0[r];
                acc[r + 4] += bf2f((bf16_t)xv[r + 4]) * w1[r];
            }
        }
        float v[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            v[r] = acc[r] + bias[c + r];
            if (GELU) v[r] = erf_gelu(v[r]);
        }
        uint4 o;
        o.x = pack_bf2(v[0], v[1]); o.y = pack_bf2(v[2], v[3]); o.z = pack_bf2(v[4], v[5]); o.w = pack_bf2(v[6], v[7]);
        *(uint4*)(out + (size_t)m * C + c) = o;
    }
}

// LayerNorm of bf16 rows [M][C] -> bf16, one wave per row (C % 8 == 0, C <= 2048)
__global__ __launch_bounds__(256) void tv_ln_kernel(const bf16_t* __restrict__ x, const float* __restrict__ g,
                                                    const float* __restrict__ b, bf16_t* __restrict__ out, int M, int C, float eps) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= M) return;
    const bf16_t* xr = x + (size_t)row * C;
    float v[4][8];
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = (lane + 64 * j) * 8;
        if (c < C) {
            const bf16x8 xv = *(const bf16x8*)(xr + c);
#pragma unroll
            for (int r = 0; r < 8; ++r) { v[j][r] = bf2f((bf16_t)xv[r]); s += v[j][r]; }
        }
    }
    const float mean = wave_sum(s) / (float)C;
    float q = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
        if ((lane + 64 * j) * 8 < C) {
#pragma unroll
            for (int r = 0; r < 8; ++r) { const float d = v[j][r] - mean; q += d * d; }
        }
    const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)C + eps);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int c = (lane + 64 * j) * 8;
        if (c < C) {
            float y[8];
#pragma unroll
            for (int r = 0; r < 8; ++r) y[r] = (v[j][r] - mean) * rstd * g[c + r] + b[c + r];
            uint4 o;
            o.x = pack_bf2(y[0], y[1]); o.y = pack_bf2(y[2], y[3]); o.z = pack_bf2(y[4], y[5]); o.w = pack_bf2(y[6], y[7]);
            *(uint4*)(out + (size_t)row * C + c) = o;
        }
    }
}

// Windowed attention.  qkv rows [n*H*W][3C], per-head interleaved: head h's q | k | v are columns h*96 + {0, 32, 64} .. +32.
// blockIdx.x = window (frame-major, then window rows, then window columns), blockIdx.y = head; thread i = query i of the
// window (token (i / ws, i % ws)), N = ws * ws <= 196.  bias: dense [heads][N][N] fp32.  ctx rows [n*H*W][C], head h at columns h*32.
__global__ __launch_bounds__(256) void tv_attn_kernel(const bf16_t* __restrict__ qkv, const float* __restrict__ bias,
                                                      bf16_t* __restrict__ ctx, int H, int W, int C, int ws, float scale) {
    __shared__ float ks[196][32];          // read as broadcasts (every thread the same key): no padding needed
    __shared__ float vs[196][32];
    const int N = ws * ws, nwx = W / ws, nwy = H / ws;
    const int win = blockIdx.x, h = blockIdx.y, heads = gridDim.y;
    const int f = win / (nwy * nwx), wy = (win / nwx) % nwy, wx = win % nwx;
    auto row_of = [&](int i) { return ((size_t)f * H + wy * ws + i / ws) * W + wx * ws + i % ws; };
    for (int e = threadIdx.x; e < N * 8; e += blockDim.x) {
        const int i = e >> 3, c = (e & 7) * 4;
        const bf16_t* src = qkv + row_of(i) * 3 * C + h * 96 + 32;
        const uint2 kk = *(const uint2*)(src + c), vv = *(const uint2*)(src + 32 + c);
        ks[i][c] = bf2f((bf16_t)(kk.x & 0xffff)); ks[i][c + 1] = bf2f((bf16_t)(kk.x >> 16));
        ks[i][c + 2] = bf2f((bf16_t)(kk.y & 0xffff)); ks[i][c + 3] = bf2f((bf16_t)(kk.y >> 16));
        vs[i][c] = bf2f((bf16_t)(vv.x & 0xffff)); vs[i][c + 1] = bf2f((bf16_t)(vv.x >> 16));
        vs[i][c + 2] = bf2f((bf16_t)(vv.y & 0xffff)); vs[i][c + 3] = bf2f((bf16_t)(vv.y >> 16));
    }
    __syncthreads();
    const int i = threadIdx.x;
    if (i >= N) return;
    const size_t row = row_of(i);
    float q[32], o[32];
    const bf16_t* qp = qkv + row * 3 * C + h * 96;
#pragma unroll
    for (int c = 0; c < 32; c += 8) {
        const bf16x8 qv = *(const bf16x8*)(qp + c);
#pragma unroll
        for (int r = 0; r < 8; ++r) q[c + r] = bf2f((bf16_t)qv[r]);
    }
#pragma unroll
    for (int d = 0; d < 32; ++d) o[d] = 0.f;
    const float* br = bias + ((size_t)h * N + i) * N;
    float mx = -INFINITY, l = 0.f;
    for (int j = 0; j < N; ++j) {
        float s = 0.f;
#pragma unroll
        for (int d = 0; d < 32; ++d) s += q[d] * ks[j][d];
        s = s * scale + br[j];
        if (s > mx) {                      // running max: rescale what was summed so far
            const float corr = __expf(mx - s);
            l *= corr;
#pragma unroll
            for (int d = 0; d < 32; ++d) o[d] *= corr;
            mx = s;
        }
        const float p = __expf(s - mx);
        l += p;
#pragma unroll
        for (int d = 0; d < 32; ++d) o[d] += p * vs[j][d];
    }
    const float inv = 1.0f / l;
    bf16_t* op = ctx + row * C + h * 32;
#pragma unroll
    for (int c = 0; c < 32; c += 8) {
        uint4 w;
        w.x = pack_bf2(o[c] * inv, o[c + 1] * inv); w.y = pack_bf2(o[c + 2] * inv, o[c + 3] * inv);
        w.z = pack_bf2(o[c + 4] * inv, o[c + 5] * inv); w.w = pack_bf2(o[c + 6] * inv, o[c + 7] * inv);
        *(uint4*)(op + c) = w;
    }
    (void)heads;
}

// memory[f][c] = (sum over pixels p = 0 .. HW-1 of x[f][p][c]) / HW
__global__ __launch_bounds__(256) void tv_pool_kernel(const bf16_t* __restrict__ x, float* __restrict__ mem, int HW, int C) {
    const int f = blockIdx.x;
    for (int c = threadIdx.x; c < C; c += 256) {
        float s = 0.f;
        for (int p = 0; p < HW; ++p) s += bf2f(x[((size_t)f * HW + p) * C + c]);
        mem[(size_t)f * C + c] = s / (float)HW;
    }
}

__global__ __launch_bounds__(256) void tv_to_nchw_kernel(const bf16_t* __restrict__ x, float* __restrict__ out, int n, int HW, int C) {
    const int64_t total = (int64_t)n * HW * C;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int p = (int)(e % HW), c = (int)((e / HW) % C);
        const int64_t f = e / ((int64_t)HW * C);
        out[e] = bf2f(x[((size_t)f * HW + p) * C + c]);
    }
}

int grid_for(int64_t total) { return (int)std::min<int64_t>((total + 255) / 256, 65536); }

hipError_t tv_gemm(const TvGemmArgs& a, int epi, hipStream_t s) {
    if (a.M <= 0 || a.N <= 0 || a.N % 4 || a.K <= 0 || a.K % 32 || a.lda % 8) return hipErrorInvalidValue;
    const dim3 grid((a.M + 31) / 32, (a.N + 31) / 32);
    switch (epi) {
        case 0: hipLaunchKernelGGL(tv_gemm_kernel<0>, grid, dim3(64), 0, s, a); break;
        case TV_GELU: hipLaunchKernelGGL(tv_gemm_kernel<TV_GELU>, grid, dim3(64), 0, s, a); break;
        case TV_RES: hipLaunchKernelGGL(tv_gemm_kernel<TV_RES>, grid, dim3(64), 0, s, a); break;
        case TV_RES | TV_RES_GELU: hipLaunchKernelGGL((tv_gemm_kernel<TV_RES | TV_RES_GELU>), grid, dim3(64), 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ---- host side ---------------------------------------------------------------------------------------------------------
struct TvConv { const bf16_t* w = nullptr; const float* dw = nullptr; const float* b = nullptr; };
struct TvBlock {            // stage 0: MBConv (c1, c2 depthwise, c3); stages 1-3: attention block
    TvConv c1, c2, c3;
    const float *ln1g = nullptr, *ln1b = nullptr, *ln2g = nullptr, *ln2b = nullptr, *qkvb = nullptr, *projb = nullptr,
                *fc1b = nullptr, *fc2b = nullptr, *bias_table = nullptr;
    const bf16_t *qkvw = nullptr, *projw = nullptr, *fc1w = nullptr, *fc2w = nullptr;
    TvConv local;
};

}  // namespace

struct gitcap_tinyvit : HandleCore {
    gitcap_tinyvit_config c;
    std::map<std::string, DevTensor> w;                  // kind 1: bf16 [N][Kp]; kind 2: depthwise, fp32 [9][C]
    bool finalized = false;
    int C[4] = {0, 0, 0, 0}, map[4] = {0, 0, 0, 0}, stem_k1 = 0, stem_k2 = 0;
    TvConv stem1, stem2, ds[4][3];
    std::vector<TvBlock> blocks[4];
    std::vector<float*> tables;                          // dense [heads][N][N] attention-bias tables (finalize)
    bf16_t *col = nullptr, *s1 = nullptr, *x = nullptr, *y = nullptr, *xn = nullptr, *t1 = nullptr, *t2 = nullptr;
};

namespace {

// the checks of gitcap_tinyvit_create; fills the stage widths and maps.  Empty string = valid.
std::string tinyvit_check(const gitcap_tinyvit_config& c, int C[4], int map[4]) {
    if (c.img_size <= 0 || c.img_size % 4) return "img_size must be a positive multiple of 4";
    if (c.max_frames <= 0) return "max_frames must be positive";
    if (!(c.ln_eps > 0.f)) return "ln_eps must be positive";
    int m = c.img_size / 4;
    for (int i = 0; i < 4; ++i) {
        C[i] = c.embed_dims[i];
        if (C[i] <= 0 || C[i] % 32 || C[i] > 2048) return "embed_dims must be multiples of 32 (<= 2048)";
        if (c.depths[i] <= 0) return "depths must be positive";
        if (i > 0) {
            if (c.merge_strides[i] != 1 && c.merge_strides[i] != 2) return "merge_strides[1..3] must be 1 or 2";
            if (c.merge_strides[i] == 2 && m % 2) return "a stride-2 merge needs an even map";
            m /= c.merge_strides[i];
            if (c.num_heads[i] <= 0 || C[i] != 32 * c.num_heads[i]) return "head_dim must be 32 (embed_dims[i] == 32 * num_heads[i])";
            if (c.window_sizes[i] <= 0 || c.window_sizes[i] > 14) return "window_sizes[1..3] must be in 1..14";
            if (m % c.window_sizes[i]) return "stage map not divisible by its window (padding is not supported)";
        }
        map[i] = m;
    }
    if (C[0] % 2 || (C[0] / 2) % 4) return "embed_dims[0] / 2 must be a multiple of 4";
    return "";
}

// dense [heads][N][N] bias table of a ws x ws window (N = ws * ws) from the checkpoint's compact [heads][N] one: entry (p, q) is
// attention_biases[h][idx(p, q)], idx = the order in which (|dy|, |dx|) first appears over points x points in row-major order
std::vector<float> tv_dense_bias_table(const float* ab, int heads, int ws) {
    const int N = ws * ws;
    std::vector<int> idx((size_t)N * N);
    std::map<std::pair<int, int>, int> first;
    for (int p = 0; p < N; ++p)
        for (int q = 0; q < N; ++q) {
            const std::pair<int, int> off(std::abs(p / ws - q / ws), std::abs(p % ws - q % ws));
            auto f = first.find(off);
            const int id = f == first.end() ? (int)first.size() : f->second;
            if (f == first.end()) first[off] = id;
            idx[(size_t)p * N + q] = id;
        }
    std::vector<float> dense((size_t)heads * N * N);
    for (int hh = 0; hh < heads; ++hh)
        for (int e = 0; e < N * N; ++e) dense[(size_t)hh * N * N + e] = ab[(size_t)hh * N + idx[e]];
    return dense;
}

}  // namespace

extern "C" {

const char* gitcap_tinyvit_last_error(const gitcap_tinyvit_t* h) { return h ? h->err.c_str() : create_err<gitcap_tinyvit>().c_str(); }

int gitcap_tinyvit_create(const gitcap_tinyvit_config* cfg, int device, gitcap_tinyvit_t** out) {
    if (!cfg || !out) return fail<gitcap_tinyvit>(nullptr, GITCAP_ERR_ARG, "tinyvit_create: null argument");
    int C[4], map[4];
    const std::string bad = tinyvit_check(*cfg, C, map);
    if (!bad.empty()) return fail<gitcap_tinyvit>(nullptr, GITCAP_ERR_ARG, "tinyvit_create: " + bad);
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail<gitcap_tinyvit>(nullptr, GITCAP_ERR_HIP, "tinyvit_create: no such HIP device (libgitcap has no CPU fallback)");
    gitcap_tinyvit* h = new gitcap_tinyvit();
    h->c = *cfg; h->device = device;
    for (int i = 0; i < 4; ++i) { h->C[i] = C[i]; h->map[i] = map[i]; }
    const int c0h = C[0] / 2;
    h->stem_k1 = pad_to(3 * 9, 32);
    h->stem_k2 = pad_to(c0h * 9, 32);
    auto add = [&](const std::string& n, std::vector<int64_t> shape, int kind) {
        DevTensor t;
        t.shape = std::move(shape);
        t.kind = kind;
        h->w[n] = t;
    };
    auto convnorm = [&](const std::string& p, int64_t cout, int64_t cin, int64_t k, bool dw) {
        add(p + ".weight", {cout, dw ? 1 : cin, k, k}, dw ? 2 : 1);
        add(p + ".bias", {cout}, 0);
    };
    auto linear = [&](const std::string& p, int64_t nout, int64_t nin) { add(p + ".weight", {nout, nin}, 1); add(p + ".bias", {nout}, 0); };
    auto norm = [&](const std::string& p, int64_t d) { add(p + ".weight", {d}, 0); add(p + ".bias", {d}, 0); };
    convnorm("patch_embed.conv1", c0h, 3, 3, false);
    convnorm("patch_embed.conv2", C[0], c0h, 3, false);
    for (int i = 0; i < 4; ++i) {
        const std::string sp = "stages_" + std::to_string(i) + ".";
        const int64_t c = C[i];
        if (i > 0) {
            convnorm(sp + "downsample.conv1", c, C[i - 1], 1, false);
            convnorm(sp + "downsample.conv2", c, c, 3, true);
            convnorm(sp + "downsample.conv3", c, c, 1, false);
        }
        for (int j = 0; j < cfg->depths[i]; ++j) {
            const std::string bp = sp + "blocks." + std::to_string(j) + ".";
            if (i == 0) {
                convnorm(bp + "conv1", 4 * c, c, 1, false);
                convnorm(bp + "conv2", 4 * c, 4 * c, 3, true);
                convnorm(bp + "conv3", c, 4 * c, 1, false);
            } else {
                const int64_t ws = cfg->window_sizes[i];
                norm(bp + "attn.norm", c);
                linear(bp + "attn.qkv", 3 * c, c);
                linear(bp + "attn.proj", c, c);
                add(bp + "attn.attention_biases", {cfg->num_heads[i], ws * ws}, 0);
                convnorm(bp + "local_conv", c, c, 3, true);
                norm(bp + "mlp.norm", c);
                linear(bp + "mlp.fc1", 4 * c, c);
                linear(bp + "mlp.fc2", c, 4 * c);
            }
        }
    }
    *out = h;
    return 0;
}

void gitcap_tinyvit_destroy(gitcap_tinyvit_t* h) {
    if (!h) return;
    DeviceGuard g(h->device);
    for (auto& kv : h->w)
        if (kv.second.p) (void)hipFree(kv.second.p);
    for (float* p : h->tables) (void)hipFree(p);
    free_allocs(*h);
    delete h;
}

int gitcap_tinyvit_load_tensor(gitcap_tinyvit_t* h, const char* name, const float* data, const int64_t* shape, int rank) {
    if (!h || !name || !data || !shape) return fail(h, GITCAP_ERR_ARG, "tinyvit_load_tensor: null argument");
    std::string why;
    DevTensor* tp = find_tensor(h->w, name, shape, rank, "tinyvit_load_tensor", why);
    if (!tp) return fail(h, GITCAP_ERR_ARG, why);
    GUARD(h);
    DevTensor& t = *tp;
    int64_t count = 1;
    for (int i = 0; i < rank; ++i) count *= shape[i];
    if (t.p) { (void)hipFree(t.p); t.p = nullptr; }
    if (t.kind == 1) {          // GEMM weight: bf16 [N][Kp], K = everything after dim 0, zero-padded to a multiple of 32
        const int64_t N = shape[0], K = count / N;
        if (int rc = upload_bf16_panel(h, t, data, N, K, 1, pad_to((int)K, 32))) return rc;
    } else if (t.kind == 2) {     // depthwise [C][1][3][3] -> fp32 [9][C]
        const int64_t Cn = shape[0];
        std::vector<float> hf((size_t)(9 * Cn));
        for (int64_t c = 0; c < Cn; ++c)
            for (int tp = 0; tp < 9; ++tp) hf[(size_t)(tp * Cn + c)] = data[c * 9 + tp];
        HIP_OK(h, hipMalloc(&t.p, hf.size() * 4));
        HIP_OK(h, hipMemcpy(t.p, hf.data(), hf.size() * 4, hipMemcpyHostToDevice));
    } else {
        HIP_OK(h, hipMalloc(&t.p, (size_t)count * 4));
        HIP_OK(h, hipMemcpy(t.p, data, (size_t)count * 4, hipMemcpyHostToDevice));
    }
    t.loaded = true;
    h->finalized = false;
    return 0;
}

int gitcap_tinyvit_finalize(gitcap_tinyvit_t* h) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "tinyvit_finalize: null handle");
    GUARD(h);
    for (auto& kv : h->w)
        if (!kv.second.loaded) return fail(h, GITCAP_ERR_STATE, "tinyvit_finalize: tensor '" + kv.first + "' was never loaded");
    auto P = [&](const std::string& n) { return h->w[n].p; };
    auto conv = [&](const std::string& p) {
        TvConv c;
        if (h->w[p + ".weight"].kind == 2) c.dw = (const float*)P(p + ".weight"); else c.w = (const bf16_t*)P(p + ".weight");
        c.b = (const float*)P(p + ".bias");
        return c;
    };
    for (float* p : h->tables) (void)hipFree(p);
    h->tables.clear();
    h->stem1 = conv("patch_embed.conv1");
    h->stem2 = conv("patch_embed.conv2");
    const gitcap_tinyvit_config& c = h->c;
    for (int i = 0; i < 4; ++i) {
        const std::string sp = "stages_" + std::to_string(i) + ".";
        if (i > 0)
            for (int k = 0; k < 3; ++k) h->ds[i][k] = conv(sp + "downsample.conv" + std::to_string(k + 1));
        h->blocks[i].assign(c.depths[i], TvBlock{});
        for (int j = 0; j < c.depths[i]; ++j) {
            const std::string bp = sp + "blocks." + std::to_string(j) + ".";
            TvBlock& b = h->blocks[i][j];
            if (i == 0) { b.c1 = conv(bp + "conv1"); b.c2 = conv(bp + "conv2"); b.c3 = conv(bp + "conv3"); continue; }
            b.ln1g = (const float*)P(bp + "attn.norm.weight"); b.ln1b = (const float*)P(bp + "attn.norm.bias");
            b.qkvw = (const bf16_t*)P(bp + "attn.qkv.weight"); b.qkvb = (const float*)P(bp + "attn.qkv.bias");
            b.projw = (const bf16_t*)P(bp + "attn.proj.weight"); b.projb = (const float*)P(bp + "attn.proj.bias");
            b.local = conv(bp + "local_conv");
            b.ln2g = (const float*)P(bp + "mlp.norm.weight"); b.ln2b = (const float*)P(bp + "mlp.norm.bias");
            b.fc1w = (const bf16_t*)P(bp + "mlp.fc1.weight"); b.fc1b = (const float*)P(bp + "mlp.fc1.bias");
            b.fc2w = (const bf16_t*)P(bp + "mlp.fc2.weight"); b.fc2b = (const float*)P(bp + "mlp.fc2.bias");
            const int ws = c.window_sizes[i], heads = c.num_heads[i];
            std::vector<float> ab((size_t)heads * ws * ws);
            HIP_OK(h, hipMemcpy(ab.data(), P(bp + "attn.attention_biases"), ab.size() * 4, hipMemcpyDeviceToHost));
            const std::vector<float> dense = tv_dense_bias_table(ab.data(), heads, ws);
            float* dt = nullptr;
            HIP_OK(h, hipMalloc(&dt, dense.size() * 4));
            h->tables.push_back(dt);
            HIP_OK(h, hipMemcpy(dt, dense.data(), dense.size() * 4, hipMemcpyHostToDevice));
            b.bias_table = dt;
        }
    }
    if (h->allocs.empty()) {
        const size_t n = (size_t)c.max_frames, img = (size_t)c.img_size;
        const size_t m1 = n * (img / 2) * (img / 2), m0 = n * (img / 4) * (img / 4);
        size_t act = 0, big = 0;            // largest [rows][C] activation and [rows][4C] / [rows][3C] hidden
        size_t prev_rows = m0;
        for (int i = 0; i < 4; ++i) {
            const size_t rows = n * h->map[i] * h->map[i];
            act = std::max(act, rows * h->C[i]);
            big = std::max(big, rows * 4 * (size_t)h->C[i]);
            if (i > 0) big = std::max(big, prev_rows * (size_t)h->C[i]);     // downsample conv1 output at the previous map
            prev_rows = rows;
        }
        const size_t col = std::max(m1 * h->stem_k1, m0 * h->stem_k2);
        int rc;
        if ((rc = dev_alloc(h, &h->col, col)) || (rc = dev_alloc(h, &h->s1, m1 * (h->C[0] / 2))) || (rc = dev_alloc(h, &h->x, act)) ||
            (rc = dev_alloc(h, &h->y, act)) || (rc = dev_alloc(h, &h->xn, act)) || (rc = dev_alloc(h, &h->t1, big)) ||
            (rc = dev_alloc(h, &h->t2, big)))
            return rc;
    }
    h->finalized = true;
    return 0;
}

}  // extern "C"

// frames: fp32 [n][3][img][img] (normalised), or -- raw != nullptr -- uint8 [n][H][W][3] BGR camera frames whose transform is
// fused with the gather of the first stem convolution (preproc.hip: preprocess_stem_kernel); everything behind that gather is shared
static int tinyvit_encode(gitcap_tinyvit* h, const float* frames, const uint8_t* raw, int rawH, int rawW, int n, float* memory,
                          float* const* fmaps, void* stream) {
    GUARD(h);
    hipStream_t s = (hipStream_t)stream;
    const gitcap_tinyvit_config& c = h->c;
    const int img = c.img_size, g1 = img / 2, g0 = img / 4, c0h = h->C[0] / 2;
    auto gemm = [&](const bf16_t* A, int K, const TvConv& cv, int M, int N, int epi, bf16_t* out, const bf16_t* res) -> int {
        TvGemmArgs a{A, K, cv.w, cv.b, res, N, out, N, M, N, K};
        HIP_OK(h, tv_gemm(a, epi, s));
        return 0;
    };
    auto lin = [&](const bf16_t* A, int K, const bf16_t* W, const float* b, int M, int N, int epi, bf16_t* out, const bf16_t* res) -> int {
        TvConv cv; cv.w = W; cv.b = b;
        return gemm(A, K, cv, M, N, epi, out, res);
    };
    auto dw = [&](const bf16_t* in, const TvConv& cv, int H, int C, int stride, bool gelu, bf16_t* out) -> int {
        const int Ho = H / stride;
        const int64_t total = (int64_t)n * Ho * Ho * (C / 8);
        if (gelu) hipLaunchKernelGGL(tv_dwconv_kernel<true>, dim3(grid_for(total)), dim3(256), 0, s, in, cv.dw, cv.b, out, n, H, H, C, stride, Ho, Ho);
        else hipLaunchKernelGGL(tv_dwconv_kernel<false>, dim3(grid_for(total)), dim3(256), 0, s, in, cv.dw, cv.b, out, n, H, H, C, stride, Ho, Ho);
        HIP_OK(h, hipGetLastError());
        return 0;
    };
    auto ln = [&](const bf16_t* in, const float* g, const float* b, int M, int C, bf16_t* out) -> int {
        hipLaunchKernelGGL(tv_ln_kernel, dim3((M + 3) / 4), dim3(256), 0, s, in, g, b, out, M, C, c.ln_eps);
        HIP_OK(h, hipGetLastError());
        return 0;
    };
    auto emit = [&](int i, const bf16_t* x) -> int {
        if (!fmaps || !fmaps[i]) return 0;
        const int HW = h->map[i] * h->map[i];
        hipLaunchKernelGGL(tv_to_nchw_kernel, dim3(grid_for((int64_t)n * HW * h->C[i])), dim3(256), 0, s, x, fmaps[i], n, HW, h->C[i]);
        HIP_OK(h, hipGetLastError());
        return 0;
    };
    int rc;
    // stem (patch_embed): conv1 3 -> C0/2 (3x3 s2) + GELU, conv2 C0/2 -> C0 (3x3 s2)
    if (raw) {
        const hipError_t e = launch_preprocess_stem(raw, h->col, n, rawH, rawW, img, s);
        if (e == hipErrorInvalidValue)
            return fail(h, GITCAP_ERR_ARG, "tinyvit_encode_raw: frame size the transform refuses (empty, or resized below img_size)");
        HIP_OK(h, e);
    } else {
        hipLaunchKernelGGL(tv_im2col_kernel<true>, dim3(grid_for((int64_t)n * g1 * g1 * h->stem_k1)), dim3(256), 0, s, frames, h->col, n,
                           img, img, 3, g1, g1, h->stem_k1);
        HIP_OK(h, hipGetLastError());
    }
    if ((rc = gemm(h->col, h->stem_k1, h->stem1, n * g1 * g1, c0h, TV_GELU, h->s1, nullptr))) return rc;
    hipLaunchKernelGGL(tv_im2col_kernel<false>, dim3(grid_for((int64_t)n * g0 * g0 * h->stem_k2)), dim3(256), 0, s, h->s1, h->col, n,
                       g1, g1, c0h, g0, g0, h->stem_k2);
    HIP_OK(h, hipGetLastError());
    bf16_t *x = h->x, *y = h->y;
    if ((rc = gemm(h->col, h->stem_k2, h->stem2, n * g0 * g0, h->C[0], 0, x, nullptr))) return rc;
    // stage 0: MBConv blocks, x = GELU(x + conv3(GELU(dw(GELU(conv1(x))))))
    {
        const int C = h->C[0], M = n * g0 * g0;
        for (const TvBlock& b : h->blocks[0]) {
            if ((rc = gemm(x, C, b.c1, M, 4 * C, TV_GELU, h->t1, nullptr))) return rc;
            if ((rc = dw(h->t1, b.c2, g0, 4 * C, 1, true, h->t2))) return rc;
            if ((rc = gemm(h->t2, 4 * C, b.c3, M, C, TV_RES | TV_RES_GELU, x, x))) return rc;
        }
        if ((rc = emit(0, x))) return rc;
    }
    for (int i = 1; i < 4; ++i) {
        const int Cp = h->C[i - 1], C = h->C[i], Hp = h->map[i - 1], H = h->map[i], st = c.merge_strides[i];
        const int M = n * H * H, ws = c.window_sizes[i], heads = c.num_heads[i];
        // PatchMerging: conv1 1x1 + GELU, depthwise 3x3 stride st + GELU, conv3 1x1
        if ((rc = gemm(x, Cp, h->ds[i][0], n * Hp * Hp, C, TV_GELU, h->t1, nullptr))) return rc;
        if ((rc = dw(h->t1, h->ds[i][1], Hp, C, st, true, h->t2))) return rc;
        if ((rc = gemm(h->t2, C, h->ds[i][2], M, C, 0, x, nullptr))) return rc;
        for (const TvBlock& b : h->blocks[i]) {
            // x = x + proj(attn(LN(x)))
            if ((rc = ln(x, b.ln1g, b.ln1b, M, C, h->xn))) return rc;
            if ((rc = lin(h->xn, C, b.qkvw, b.qkvb, M, 3 * C, 0, h->t1, nullptr))) return rc;
            hipLaunchKernelGGL(tv_attn_kernel, dim3(n * (H / ws) * (H / ws), heads), dim3((ws * ws + 63) / 64 * 64), 0, s, h->t1,
                               b.bias_table, h->t2, H, H, C, ws, 0.17677669529663687f);
            HIP_OK(h, hipGetLastError());
            if ((rc = lin(h->t2, C, b.projw, b.projb, M, C, TV_RES, x, x))) return rc;
            // x = local_conv(x): depthwise 3x3 + BN, no residual, no activation
            if ((rc = dw(x, b.local, H, C, 1, false, y))) return rc;
            std::swap(x, y);
            // x = x + fc2(GELU(fc1(LN(x))))
            if ((rc = ln(x, b.ln2g, b.ln2b, M, C, h->xn))) return rc;
            if ((rc = lin(h->xn, C, b.fc1w, b.fc1b, M, 4 * C, TV_GELU, h->t1, nullptr))) return rc;
            if ((rc = lin(h->t1, 4 * C, b.fc2w, b.fc2b, M, C, TV_RES, x, x))) return rc;
        }
        if ((rc = emit(i, x))) return rc;
    }
    hipLaunchKernelGGL(tv_pool_kernel, dim3(n), dim3(256), 0, s, x, memory, h->map[3] * h->map[3], h->C[3]);
    HIP_OK(h, hipGetLastError());
    return 0;
}

extern "C" {

int gitcap_tinyvit_encode(gitcap_tinyvit_t* h, const float* frames, int n, float* memory, float* const* fmaps, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "tinyvit_encode: null handle");
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "tinyvit_encode: weights not finalized");
    if (!frames || !memory || n <= 0) return fail(h, GITCAP_ERR_ARG, "tinyvit_encode: bad arguments");
    if (n > h->c.max_frames) return fail(h, GITCAP_ERR_ARG, "tinyvit_encode: n exceeds max_frames");
    return tinyvit_encode(h, frames, nullptr, 0, 0, n, memory, fmaps, stream);
}

int gitcap_tinyvit_encode_raw(gitcap_tinyvit_t* h, const uint8_t* frames_hwc_bgr, int n, int H, int W, float* memory,
                              float* const* fmaps, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "tinyvit_encode_raw: null handle");
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "tinyvit_encode_raw: weights not finalized");
    if (!frames_hwc_bgr || !memory || n <= 0 || H <= 0 || W <= 0) return fail(h, GITCAP_ERR_ARG, "tinyvit_encode_raw: bad arguments");
    if (n > h->c.max_frames) return fail(h, GITCAP_ERR_ARG, "tinyvit_encode_raw: n exceeds max_frames");
    if ((int64_t)n * H * W * 3 > ((int64_t)1 << 40)) return fail(h, GITCAP_ERR_ARG, "tinyvit_encode_raw: sizes overflow");
    return tinyvit_encode(h, nullptr, frames_hwc_bgr, H, W, n, memory, fmaps, stream);
}

// ---- kernel-level test hooks (tests/test_encoder_kernels_gpu.py): each launches ONE kernel of this file (attn_small: of
// student.hip) on caller-owned device buffers, no handle; what a wrong value of would index outside a buffer or misalign a vector
// access is refused here, before any launch
static bool misaligned(const void* p, uintptr_t bytes) { return ((uintptr_t)p & (bytes - 1)) != 0; }

int gitcap_dbg_tv_gemm(const void* A, int lda, const void* W, const float* bias, const void* res, int ldr, void* out, int ldo, int M,
                       int N, int K, int epi, void* stream) {
    if (!A || !W || !bias || !out || M <= 0 || N <= 0 || (N & 3) || K <= 0 || (K & 31) || lda < K || (lda & 7) || ldo < N || (ldo & 3) ||
        (ldr & 3))
        return GITCAP_ERR_ARG;
    if (epi != 0 && epi != TV_GELU && epi != TV_RES && epi != (TV_RES | TV_RES_GELU)) return GITCAP_ERR_ARG;
    if ((epi & TV_RES) && (!res || ldr < N || misaligned(res, 8))) return GITCAP_ERR_ARG;
    if (misaligned(A, 16) || misaligned(W, 16) || misaligned(bias, 16) || misaligned(out, 8)) return GITCAP_ERR_ARG;
    const TvGemmArgs a{(const bf16_t*)A, lda, (const bf16_t*)W, bias, (const bf16_t*)res, ldr, (bf16_t*)out, ldo, M, N, K};
    return dbg_rc(tv_gemm(a, epi, (hipStream_t)stream));
}

int gitcap_dbg_tv_im2col(const void* in, int f32_nchw, void* out, int n, int H, int W, int Cin, int Kp, void* stream) {
    if (!in || !out || n <= 0 || H <= 0 || W <= 0 || (H & 1) || (W & 1) || Cin <= 0 || Kp < 9 * Cin || misaligned(in, f32_nchw ? 4 : 2) ||
        misaligned(out, 2))
        return GITCAP_ERR_ARG;
    const int Ho = H / 2, Wo = W / 2;
    const dim3 grid(grid_for((int64_t)n * Ho * Wo * Kp));
    if (f32_nchw) hipLaunchKernelGGL(tv_im2col_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, in, (bf16_t*)out, n, H, W, Cin, Ho, Wo, Kp);
    else hipLaunchKernelGGL(tv_im2col_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, in, (bf16_t*)out, n, H, W, Cin, Ho, Wo, Kp);
    return dbg_rc(hipGetLastError());
}

int gitcap_dbg_tv_dwconv(const void* x, const float* w9, const float* bias, void* out, int n, int H, int W, int C, int stride, int gelu,
                         void* stream) {
    if (!x || !w9 || !bias || !out || n <= 0 || H <= 0 || W <= 0 || C <= 0 || (C & 7) || (stride != 1 && stride != 2) ||
        (stride == 2 && ((H & 1) || (W & 1))) || misaligned(x, 16) || misaligned(w9, 16) || misaligned(bias, 4) || misaligned(out, 16))
        return GITCAP_ERR_ARG;
    const int Ho = H / stride, Wo = W / stride;
    const dim3 grid(grid_for((int64_t)n * Ho * Wo * (C / 8)));
    if (gelu) hipLaunchKernelGGL(tv_dwconv_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, w9, bias, (bf16_t*)out, n, H, W, C, stride, Ho, Wo);
    else hipLaunchKernelGGL(tv_dwconv_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, w9, bias, (bf16_t*)out, n, H, W, C, stride, Ho, Wo);
    return dbg_rc(hipGetLastError());
}

int gitcap_dbg_tv_ln(const void* x, const float* g, const float* b, void* out, int M, int C, float eps, void* stream) {
    if (!x || !g || !b || !out || M <= 0 || C <= 0 || (C & 7) || C > 2048 || misaligned(x, 16) || misaligned(g, 4) || misaligned(b, 4) ||
        misaligned(out, 16))
        return GITCAP_ERR_ARG;
    hipLaunchKernelGGL(tv_ln_kernel, dim3((M + 3) / 4), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, g, b, (bf16_t*)out, M, C, eps);
    return dbg_rc(hipGetLastError());
}

// attention_biases: the compact checkpoint table, device fp32 [heads][ws * ws]; the dense table the kernel reads is built as
// gitcap_tinyvit_finalize builds it and lives until the launch has finished (the call synchronises `stream`)
int gitcap_dbg_tv_attn(const void* qkv, const float* attention_biases, void* ctx, int n, int H, int W, int heads, int ws, void* stream) {
    if (!qkv || !attention_biases || !ctx || n <= 0 || heads <= 0 || ws < 1 || ws > 14 || H <= 0 || W <= 0 || H % ws || W % ws ||
        misaligned(qkv, 16) || misaligned(attention_biases, 4) || misaligned(ctx, 16))
        return GITCAP_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int N = ws * ws;
    std::vector<float> ab((size_t)heads * N);
    if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(ab.data(), attention_biases, ab.size() * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return GITCAP_ERR_HIP;
    const std::vector<float> dense = tv_dense_bias_table(ab.data(), heads, ws);
    float* dt = nullptr;
    if (hipMalloc(&dt, dense.size() * 4) != hipSuccess) return GITCAP_ERR_NOMEM;
    hipError_t e = hipMemcpy(dt, dense.data(), dense.size() * 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(tv_attn_kernel, dim3(n * (H / ws) * (W / ws), heads), dim3((N + 63) / 64 * 64), 0, s, (const bf16_t*)qkv, dt,
                           (bf16_t*)ctx, H, W, heads * 32, ws, 0.17677669529663687f);
        e = hipGetLastError();
    }
    const hipError_t es = hipStreamSynchronize(s);
    (void)hipFree(dt);
    return dbg_rc(e != hipSuccess ? e : es);
}

int gitcap_dbg_tv_pool(const void* x, float* mem, int n, int HW, int C, void* stream) {
    if (!x || !mem || n <= 0 || HW <= 0 || C <= 0 || misaligned(x, 2) || misaligned(mem, 4)) return GITCAP_ERR_ARG;
    hipLaunchKernelGGL(tv_pool_kernel, dim3(n), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, mem, HW, C);
    return dbg_rc(hipGetLastError());
}

int gitcap_dbg_tv_to_nchw(const void* x, float* out, int n, int HW, int C, void* stream) {
    if (!x || !out || n <= 0 || HW <= 0 || C <= 0 || misaligned(x, 2) || misaligned(out, 4)) return GITCAP_ERR_ARG;
    hipLaunchKernelGGL(tv_to_nchw_kernel, dim3(grid_for((int64_t)n * HW * C)), dim3(256), 0, (hipStream_t)stream, (const bf16_t*)x, out, n, HW, C);
    return dbg_rc(hipGetLastError());
}

// the student decoder's attention (student.hip: attn_small_kernel) through its launcher; the struct mirrors SmallAttnArgs
int gitcap_dbg_attn_small(const gitcap_dbg_attn_small_args* g, void* stream) {
    if (!g || !g->q || !g->k || !g->v || !g->ctx || g->T <= 0 || g->M <= 0 || g->M % g->T || g->H <= 0 || g->hd <= 0 || g->nkeys < 0 ||
        g->t0 < 0 || g->q_row_stride < 0 || g->q_row_off < 0 || g->keys_stride < 0 || g->ldq < g->H * g->hd || g->ldkv < g->H * g->hd ||
        (g->ldkv & 7) || g->ldc < g->H * g->hd || (g->ids && g->ld_ids < (g->nkeys > 0 ? g->nkeys : g->t0 + g->T)) || misaligned(g->q, 2) ||
        misaligned(g->k, 16) || misaligned(g->v, 2) || misaligned(g->ids, 8) || misaligned(g->ctx, 2))
        return GITCAP_ERR_ARG;
    const SmallAttnArgs a{(const bf16_t*)g->q, g->ldq, g->T, g->q_row_stride, g->q_row_off, (const bf16_t*)g->k, (const bf16_t*)g->v,
                          g->ldkv, g->keys_stride, g->nkeys, g->t0, g->ids, g->ld_ids, g->pad_id, (bf16_t*)g->ctx, g->ldc, g->M, g->H, g->hd};
    return dbg_rc(launch_attn_small(a, (hipStream_t)stream));
}

// its variable-length form (attn_small_kernel<true>): key_off / key_len device int32 [M / T]; nkeys, keys_stride and t0 of the struct
// are not read and ids must be null.  The tables are read back first (the call synchronises `stream`): a length outside [1, 64] or a
// negative offset is refused before any launch.
int gitcap_dbg_attn_small_varlen(const gitcap_dbg_attn_small_args* g, const int32_t* key_off, const int32_t* key_len, void* stream) {
    if (!g || !g->q || !g->k || !g->v || !g->ctx || !key_off || !key_len || g->ids || g->T <= 0 || g->M <= 0 || g->M % g->T || g->H <= 0 ||
        g->hd <= 0 || g->q_row_stride < 0 || g->q_row_off < 0 || g->ldq < g->H * g->hd || g->ldkv < g->H * g->hd || (g->ldkv & 7) ||
        g->ldc < g->H * g->hd || misaligned(g->q, 2) || misaligned(g->k, 16) || misaligned(g->v, 2) || misaligned(g->ctx, 2) ||
        misaligned(key_off, 4) || misaligned(key_len, 4))
        return GITCAP_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    const int rows = g->M / g->T;
    std::vector<int32_t> tab(2 * (size_t)rows);
    if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(tab.data(), key_off, (size_t)rows * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(tab.data() + rows, key_len, (size_t)rows * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return GITCAP_ERR_HIP;
    for (int r = 0; r < rows; ++r)
        if (tab[r] < 0 || tab[rows + r] < 1 || tab[rows + r] > 64) return GITCAP_ERR_ARG;
    const SmallAttnArgs a{(const bf16_t*)g->q, g->ldq, g->T, g->q_row_stride, g->q_row_off, (const bf16_t*)g->k, (const bf16_t*)g->v,
                          g->ldkv, 0, 0, 0, nullptr, 0, 0, (bf16_t*)g->ctx, g->ldc, g->M, g->H, g->hd};
    return dbg_rc(launch_attn_small_varlen(a, key_off, key_len, s));
}

}  // extern "C"
