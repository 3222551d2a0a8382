// Frame sampling of whole decoded videos on the device (include/gitcap.h: gitcap_frame_chain, gitcap_frame_features, gitcap_kmeans,
// gitcap_frame_select), the device side of gitcap.sampling.  Replaces the reference's content-driven frame samplers
// (src/utils/frame_sampling_methods.py:135-297): the two sequential ones (keep a frame when it is far enough from the last frame
// kept, by mean squared error or by the chi-square distance of histograms) and the clustered one (k-means over downsampled frames,
// keep a frame when its cluster differs from the previous frame's).
//
// Nothing here waits on another workgroup: every step is a kernel of its own and the steps are ordered by the stream alone.  What
// a later step needs from an earlier one -- which frame is the chain's reference, whether k-means has converged -- is a word in
// the call's scratch (a stream-ordered allocation of the call), written by one thread of one kernel and read by the kernels
// enqueued behind it.  So all steps of a call are enqueued back to back and the host never looks at an intermediate result.
//
//   * gate chain: step i compares frame i with frame ref_idx.  The pair pass is frame_change_kernel's (framegate.hip), restated
//     here with the reference pointer read from the scratch: packed 8-bit dot products, wave-private LDS histograms, a 64-bit sum;
//     the aligned / byte-wise / tail split depends on both addresses and is decided in the kernel (uniform: every thread loads
//     the same ref_idx).  The finalize has frame_change_finalize_kernel's fp64 operation order, so dist[i] is bit for bit what
//     gitcap_frame_change gives for the pair; it also takes the decision, moves ref_idx and zeroes the sums for the next step.
//   * features: bilinear downsample with half-pixel centres; the source coordinate is an exact integer quotient, so the only
//     roundings are the two weights' and the four products and three additions of the blend (no rounding back to uint8).
//   * k-means: Lloyd's algorithm with every iteration enqueued up front.  assign: one workgroup per frame, the direct
//     sum_d (x_d - c_d)^2 in fp32 in a fixed order, ties to the lower cluster; it counts the changed labels of its iteration into
//     a word of that iteration.  update: a thread per (cluster, dimension) adds the cluster's rows in ascending order -- no float
//     atomics, two runs are bit-identical; a cluster without rows keeps its centroid.  The update of an iteration that changed no
//     label sets `done`; every later assign returns on it, and so does every later update on its iteration's untouched count.
//   * selection: one workgroup scans the keep flags (or the labels' run boundaries) into ascending indices and thins them to
//     max_frames.
#include "../../include/gitcap.h"
#include "kernels.h"

namespace {

// ------------------------------------------------------------------------------------------------------------------ gate chain
constexpr int FC_THREADS = 256, FC_WAVES = FC_THREADS / 64;
constexpr int FC_CHUNK = 48;                 // as framegate.hip: three 16-byte loads, a whole number of BGR triples
constexpr int FC_CHUNKS_PER_THREAD = 4;
constexpr int FC_MAX_BLOCKS = 256;

// scratch of one chain: the sums of the step in flight and the reference frame's index
struct ChainScratch {
    unsigned long long ssd;
    int ref_idx;
    int pad;
    unsigned hist[2][256];                   // 0 = frame, 1 = ref
};

__device__ __forceinline__ unsigned sq_diff4(unsigned a, unsigned b) {
    const unsigned aa = __builtin_amdgcn_udot4(a, a, 0u, false), bb = __builtin_amdgcn_udot4(b, b, 0u, false);
    return aa + bb - 2u * __builtin_amdgcn_udot4(a, b, 0u, false);
}

template <int SEL>
__device__ __forceinline__ unsigned fc_chunk(const uint4* __restrict__ pf, const uint4* __restrict__ pr, unsigned* hf, unsigned* hr) {
    uint4 va[3], vb[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) { va[i] = pf[i]; vb[i] = pr[i]; }
    unsigned a[12], b[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        a[4 * i] = va[i].x; a[4 * i + 1] = va[i].y; a[4 * i + 2] = va[i].z; a[4 * i + 3] = va[i].w;
        b[4 * i] = vb[i].x; b[4 * i + 1] = vb[i].y; b[4 * i + 2] = vb[i].z; b[4 * i + 3] = vb[i].w;
    }
    unsigned s = 0;
#pragma unroll
    for (int w = 0; w < 12; ++w) {
        s += sq_diff4(a[w], b[w]);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if ((4 * w + j) % 3 == SEL) {
                atomicAdd(&hf[(a[w] >> (8 * j)) & 255u], 1u);
                atomicAdd(&hr[(b[w] >> (8 * j)) & 255u], 1u);
            }
    }
    return s;
}

template <int SEL>
__device__ __forceinline__ unsigned long long fc_body(const unsigned char* __restrict__ f, const unsigned char* __restrict__ r,
                                                      int64_t chunks, unsigned* hf, unsigned* hr) {
    unsigned long long s = 0;
    for (int64_t c = (int64_t)blockIdx.x * FC_THREADS + threadIdx.x; c < chunks; c += (int64_t)gridDim.x * FC_THREADS)
        s += fc_chunk<SEL>((const uint4*)(f + c * FC_CHUNK), (const uint4*)(r + c * FC_CHUNK), hf, hr);
    return s;
}

// one thread per frame: the outputs of frames that are never looked at, the first reference, zero sums
__global__ __launch_bounds__(256) void chain_init_kernel(int N, unsigned char* __restrict__ keep, double* __restrict__ dist,
                                                         ChainScratch* __restrict__ sc) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < N) {
        keep[i] = i == 0;
        dist[i] = __longlong_as_double(0x7ff8000000000000ll);
    }
    if (blockIdx.x == 0) {
        for (int j = threadIdx.x; j < 512; j += 256) (&sc->hist[0][0])[j] = 0u;
        if (threadIdx.x == 0) { sc->ssd = 0ull; sc->ref_idx = 0; sc->pad = 0; }
    }
}

// grid: workgroups of one step.  Frame `step` of video against frame sc->ref_idx (< step); n = H*W*3 bytes per frame.
__global__ __launch_bounds__(FC_THREADS) void chain_step_kernel(const unsigned char* __restrict__ video, int64_t n, int step, int channel,
                                                                ChainScratch* __restrict__ sc) {
    __shared__ unsigned hist[FC_WAVES][2][256];
    __shared__ unsigned long long blk_ssd;
    const int tid = threadIdx.x, wave = tid >> 6;
    for (int i = tid; i < FC_WAVES * 2 * 256; i += FC_THREADS) (&hist[0][0][0])[i] = 0u;
    if (tid == 0) blk_ssd = 0ull;
    __syncthreads();
    unsigned* hf = hist[wave][0];
    unsigned* hr = hist[wave][1];

    int ref = sc->ref_idx;
    ref = ref < 0 ? 0 : (ref >= step ? step - 1 : ref);               // the finalize only ever writes a looked-at index below `step`
    const unsigned char* f = video + (int64_t)step * n;
    const unsigned char* r = video + (int64_t)ref * n;
    // as frame_change_kernel: [0, head) up to the frame's first 16-byte boundary, `chunks` whole chunks, the rest one at a time;
    // the reference must reach its boundary with the same head, else there are no chunks.  (step - ref) * n modulo 16 changes from
    // step to step whenever n is no multiple of 16.
    int64_t head = (int64_t)((16u - (unsigned)((uintptr_t)f & 15u)) & 15u);
    if (head > n) head = n;
    int64_t chunks = (n - head) / FC_CHUNK;
    if (((uintptr_t)(r + head) & 15u) != 0) { head = 0; chunks = 0; }
    const int64_t body = chunks * FC_CHUNK;

    unsigned long long s = 0;
    switch ((channel + 3 - (int)(head % 3)) % 3) {
        case 0: s = fc_body<0>(f + head, r + head, chunks, hf, hr); break;
        case 1: s = fc_body<1>(f + head, r + head, chunks, hf, hr); break;
        default: s = fc_body<2>(f + head, r + head, chunks, hf, hr); break;
    }
    for (int64_t i = (int64_t)blockIdx.x * FC_THREADS + tid; i < n - body; i += (int64_t)gridDim.x * FC_THREADS) {
        const int64_t pos = i < head ? i : i + body;
        const unsigned a = f[pos], c = r[pos];
        const int d = (int)a - (int)c;
        s += (unsigned)(d * d);
        if ((int)(pos % 3) == channel) {
            atomicAdd(&hf[a], 1u);
            atomicAdd(&hr[c], 1u);
        }
    }

#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_down(s, o);
    if ((tid & 63) == 0) atomicAdd(&blk_ssd, s);
    __syncthreads();
    if (tid == 0) atomicAdd(&sc->ssd, blk_ssd);
#pragma unroll
    for (int k = 0; k < 2; ++k) {                          // thread = bin
        unsigned m = 0;
#pragma unroll
        for (int w = 0; w < FC_WAVES; ++w) m += hist[w][k][tid];
        if (m) atomicAdd(&sc->hist[k][tid], m);
    }
}

// one wave: the step's distance in frame_change_finalize_kernel's operation order, the decision, the next reference, zero sums
__global__ __launch_bounds__(64) void chain_finalize_kernel(ChainScratch* __restrict__ sc, int64_t n, int step, int metric, double threshold,
                                                            unsigned char* __restrict__ keep, double* __restrict__ dist) {
    __shared__ double term[256];
    const int lane = threadIdx.x;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = lane + 64 * k;
        const unsigned nf = sc->hist[0][i], nr = sc->hist[1][i];
        const long long d = (long long)nr - (long long)nf;
        term[i] = nr ? (double)(d * d) / (double)nr : 0.0;
        sc->hist[0][i] = 0u;
        sc->hist[1][i] = 0u;
    }
    __syncthreads();
    if (lane == 0) {
        double v;
        if (metric == 0) {
            v = (double)sc->ssd / (double)n;
        } else {
            double acc = 0.0;
            for (int i = 0; i < 256; ++i) acc += term[i];
            v = acc;
        }
        const bool kept = v > threshold;
        dist[step] = v;
        keep[step] = kept;
        if (kept) sc->ref_idx = step;
        sc->ssd = 0ull;
    }
}

// -------------------------------------------------------------------------------------------------------------------- features
// one thread per output element (frame, y, x, channel).  Source coordinate of output row y: ((2y + 1) H - h2) / (2 h2), not below 0,
// as an integer quotient and remainder: the tap is exact and the weight is one fp32 division of two small integers.
__global__ __launch_bounds__(256) void frame_features_kernel(const unsigned char* __restrict__ video, int N, int H, int W, int h2, int w2,
                                                             float* __restrict__ X) {
    const int64_t total = (int64_t)N * h2 * w2 * 3;
    const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= total) return;
    const int c = (int)(e % 3);
    const int x = (int)((e / 3) % w2);
    const int y = (int)((e / (3 * (int64_t)w2)) % h2);
    const int64_t fr = e / (3 * (int64_t)w2 * h2);
    int64_t ny = (int64_t)(2 * y + 1) * H - h2, nx = (int64_t)(2 * x + 1) * W - w2;
    if (ny < 0) ny = 0;
    if (nx < 0) nx = 0;
    const int y0 = (int)(ny / (2 * h2)), x0 = (int)(nx / (2 * w2));
    const int y1 = y0 + 1 < H ? y0 + 1 : H - 1, x1 = x0 + 1 < W ? x0 + 1 : W - 1;
    const float ly = (float)(int)(ny % (2 * h2)) / (float)(2 * h2), lx = (float)(int)(nx % (2 * w2)) / (float)(2 * w2);
    const float my = 1.0f - ly, mx = 1.0f - lx;
    const unsigned char* p = video + fr * (int64_t)H * W * 3 + c;
    const float a = (float)p[((int64_t)y0 * W + x0) * 3], b = (float)p[((int64_t)y0 * W + x1) * 3];
    const float g = (float)p[((int64_t)y1 * W + x0) * 3], h = (float)p[((int64_t)y1 * W + x1) * 3];
    X[e] = ((a * (my * mx) + b * (my * lx)) + g * (ly * mx)) + h * (ly * lx);
}

// --------------------------------------------------------------------------------------------------------------------- k-means
constexpr int KM_THREADS = 256, KM_WAVES = KM_THREADS / 64;
constexpr int KM_TILE = 4;                   // centroids per pass over a frame's row

// state of one call: done, then the changed-label count of every iteration (index = iteration, 1-based)
__host__ __device__ inline size_t km_state_ints(int max_iter) { return (size_t)max_iter + 2; }

// grid (D / 256, k): centroid c = row init_idx[c] (an index outside [0, N) is clamped); block (0, 0) also resets labels and state
__global__ __launch_bounds__(KM_THREADS) void kmeans_init_kernel(const float* __restrict__ X, int N, int D, const int* __restrict__ init_idx,
                                                                 int max_iter, int* __restrict__ labels, float* __restrict__ centroids,
                                                                 int* __restrict__ iters, int* __restrict__ state) {
    const int c = blockIdx.y, d = blockIdx.x * KM_THREADS + threadIdx.x;
    int row = init_idx[c];
    row = row < 0 ? 0 : (row >= N ? N - 1 : row);
    if (d < D) centroids[(size_t)c * D + d] = X[(size_t)row * D + d];
    if (blockIdx.x == 0 && c == 0) {
        for (int i = threadIdx.x; i < N; i += KM_THREADS) labels[i] = -1;
        for (size_t i = threadIdx.x; i < km_state_ints(max_iter); i += KM_THREADS) state[i] = 0;
        if (threadIdx.x == 0) *iters = max_iter;
    }
}

// grid N, one workgroup per frame.  sum_d (x_d - c_d)^2: thread t adds d = t, t + 256, ... in ascending order, a wave adds its lanes
// by halving (lane l += lane l + 32, 16, ... 1), thread 0 adds the four waves in order.  Strictly smaller wins: ties go to the lower c.
// done (may be null): return at once when set.  changed: += 1 when the label differs from the one in `labels`.
__global__ __launch_bounds__(KM_THREADS) void kmeans_assign_kernel(const float* __restrict__ X, int D, int k, const float* __restrict__ centroids,
                                                                   int* __restrict__ labels, const int* __restrict__ done, int* __restrict__ changed) {
    if (done && *done) return;
    __shared__ float red[KM_WAVES][KM_TILE];
    const int n = blockIdx.x, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const float* x = X + (size_t)n * D;
    float best = 0.0f;
    int arg = -1;
    for (int c0 = 0; c0 < k; c0 += KM_TILE) {
        const float* cp[KM_TILE];
#pragma unroll
        for (int j = 0; j < KM_TILE; ++j) cp[j] = centroids + (size_t)(c0 + j < k ? c0 + j : k - 1) * D;
        float acc[KM_TILE];
#pragma unroll
        for (int j = 0; j < KM_TILE; ++j) acc[j] = 0.0f;
        for (int d = tid; d < D; d += KM_THREADS) {
            const float xv = x[d];
#pragma unroll
            for (int j = 0; j < KM_TILE; ++j) {
                const float diff = xv - cp[j][d];
                acc[j] += diff * diff;
            }
        }
#pragma unroll
        for (int j = 0; j < KM_TILE; ++j) {
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) acc[j] += __shfl_down(acc[j], o);
            if (lane == 0) red[wave][j] = acc[j];
        }
        __syncthreads();
        if (tid == 0) {
#pragma unroll
            for (int j = 0; j < KM_TILE; ++j) {
                if (c0 + j >= k) continue;
                float v = red[0][j];
#pragma unroll
                for (int w = 1; w < KM_WAVES; ++w) v += red[w][j];
                if (arg < 0 || v < best) { best = v; arg = c0 + j; }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        if (labels[n] != arg) atomicAdd(changed, 1);
        labels[n] = arg;
    }
}

// grid (D / 256, k): centroid (c, d) = the mean of X[n][d] over the rows with labels[n] == c, added in ascending n; no such row: kept.
// state (null for the hook): the update of iteration `it` returns when that iteration changed no label (after a `done` every
// later count stays zero, so every later update returns too); the first one to see it records done and iters.
__global__ __launch_bounds__(KM_THREADS) void kmeans_update_kernel(const float* __restrict__ X, int N, int D, const int* __restrict__ labels,
                                                                   float* __restrict__ centroids, int* __restrict__ state, int it,
                                                                   int* __restrict__ iters) {
    if (state && state[1 + it] == 0) {
        if (blockIdx.x == 0 && blockIdx.y == 0 && threadIdx.x == 0 && !state[0]) { state[0] = 1; *iters = it; }
        return;
    }
    const int c = blockIdx.y, d = blockIdx.x * KM_THREADS + threadIdx.x;
    if (d >= D) return;
    float s = 0.0f;
    int m = 0;
    for (int n = 0; n < N; ++n)
        if (labels[n] == c) { s += X[(size_t)n * D + d]; ++m; }
    if (m) centroids[(size_t)c * D + d] = s / (float)m;
}

// ------------------------------------------------------------------------------------------------------------------- selection
constexpr int SEL_THREADS = 1024, SEL_WAVES = SEL_THREADS / 64;

// one workgroup.  Pass 1: kept indices in ascending order into idx[0, K) (a block scan per 1024 frames, a running base).  Pass 2, when
// K > max_frames: idx[j] = kept[floor(j K / max_frames)]; the source index is >= j, so a block of j reads before it writes and
// blocks go in ascending order.  idx[count, N) = -1.
__global__ __launch_bounds__(SEL_THREADS) void frame_select_kernel(const unsigned char* __restrict__ keep, const int* __restrict__ labels, int N,
                                                                   int max_frames, long long* __restrict__ idx, int* __restrict__ count) {
    __shared__ int wave_sum[SEL_WAVES];
    __shared__ int base;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    if (tid == 0) base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < N; i0 += SEL_THREADS) {
        const int i = i0 + tid;
        bool flag = false;
        if (i < N) flag = keep ? keep[i] != 0 : (i == 0 || labels[i] != labels[i - 1]);
        const unsigned long long mask = __ballot(flag);
        const int before = __popcll(mask & ((1ull << lane) - 1ull));
        if (lane == 0) wave_sum[wave] = __popcll(mask);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wave; ++w) off += wave_sum[w];
        if (flag) idx[off + before] = i;
        __syncthreads();
        if (tid == 0) {
            int t = base;
            for (int w = 0; w < SEL_WAVES; ++w) t += wave_sum[w];
            base = t;
        }
        __syncthreads();
    }
    const int K = base;
    const int cnt = K < max_frames ? K : max_frames;
    if (K > max_frames) {
        for (int j0 = 0; j0 < max_frames; j0 += SEL_THREADS) {
            const int j = j0 + tid;
            long long v = 0;
            if (j < max_frames) v = idx[(long long)j * K / max_frames];
            __syncthreads();
            if (j < max_frames) idx[j] = v;
            __syncthreads();
        }
    }
    for (int i = cnt + tid; i < N; i += SEL_THREADS) idx[i] = -1;
    if (tid == 0) *count = cnt;
}

inline int status(hipError_t e) { return e == hipSuccess ? 0 : GITCAP_ERR_HIP; }

}  // namespace

extern "C" {

int gitcap_frame_chain(const uint8_t* video_hwc_bgr, int N, int H, int W, int metric, int channel, double threshold, int every,
                       uint8_t* keep, double* dist, void* stream) {
    if (!video_hwc_bgr || !keep || !dist || N <= 0 || H < 1 || W < 1 || metric < 0 || metric > 1 || channel < 0 || channel > 2 || every < 1)
        return GITCAP_ERR_ARG;
    const int64_t n = (int64_t)H * W * 3;
    if (n > INT32_MAX) return GITCAP_ERR_ARG;                         // 32-bit bin counts
    hipStream_t s = (hipStream_t)stream;
    ChainScratch* sc = nullptr;
    if (hipMallocAsync((void**)&sc, sizeof(ChainScratch), s) != hipSuccess) return GITCAP_ERR_NOMEM;
    hipLaunchKernelGGL(chain_init_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, s, N, keep, dist, sc);
    hipError_t e = hipGetLastError();
    const int64_t per_block = (int64_t)FC_THREADS * FC_CHUNK * FC_CHUNKS_PER_THREAD;
    int64_t blocks = (n + per_block - 1) / per_block;
    if (blocks > FC_MAX_BLOCKS) blocks = FC_MAX_BLOCKS;
    for (int64_t i = every; i < N && e == hipSuccess; i += every) {
        hipLaunchKernelGGL(chain_step_kernel, dim3((unsigned)blocks), dim3(FC_THREADS), 0, s, video_hwc_bgr, n, (int)i, channel, sc);
        hipLaunchKernelGGL(chain_finalize_kernel, dim3(1), dim3(64), 0, s, sc, n, (int)i, metric, threshold, keep, dist);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(sc, s);
    return status(e);
}

int gitcap_frame_features(const uint8_t* video_hwc_bgr, int N, int H, int W, int h2, int w2, float* X, void* stream) {
    if (!video_hwc_bgr || !X || N <= 0 || H < 1 || W < 1 || h2 < 1 || w2 < 1 || h2 > (1 << 22) || w2 > (1 << 22)) return GITCAP_ERR_ARG;   // 2 h2 exact in fp32
    const int64_t total = (int64_t)N * h2 * w2 * 3;
    if ((int64_t)H * W * 3 > INT32_MAX || (total + 255) / 256 > INT32_MAX) return GITCAP_ERR_ARG;
    hipLaunchKernelGGL(frame_features_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, video_hwc_bgr, N, H, W,
                       h2, w2, X);
    return status(hipGetLastError());
}

int gitcap_kmeans(const float* X, int N, int D, int k, const int32_t* init_idx, int max_iter, int32_t* labels, float* centroids,
                  int32_t* iters, void* stream) {
    if (!X || !init_idx || !labels || !centroids || !iters || N <= 0 || D < 1 || k < 1 || k > N || max_iter < 1 || max_iter > (1 << 20) ||
        k > 65535)
        return GITCAP_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    int* state = nullptr;
    if (hipMallocAsync((void**)&state, km_state_ints(max_iter) * sizeof(int), s) != hipSuccess) return GITCAP_ERR_NOMEM;
    const dim3 per_centroid((unsigned)((D + KM_THREADS - 1) / KM_THREADS), (unsigned)k);
    hipLaunchKernelGGL(kmeans_init_kernel, per_centroid, dim3(KM_THREADS), 0, s, X, N, D, init_idx, max_iter, labels, centroids, iters, state);
    hipError_t e = hipGetLastError();
    for (int it = 1; it <= max_iter && e == hipSuccess; ++it) {
        hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)N), dim3(KM_THREADS), 0, s, X, D, k, (const float*)centroids, labels,
                           (const int*)state, state + 1 + it);
        hipLaunchKernelGGL(kmeans_update_kernel, per_centroid, dim3(KM_THREADS), 0, s, X, N, D, (const int*)labels, centroids, state, it, iters);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(state, s);
    return status(e);
}

int gitcap_dbg_kmeans_assign(const float* X, int N, int D, int k, const float* centroids, int32_t* labels, int32_t* changed, void* stream) {
    if (!X || !centroids || !labels || !changed || N <= 0 || D < 1 || k < 1 || k > N) return GITCAP_ERR_ARG;
    hipLaunchKernelGGL(kmeans_assign_kernel, dim3((unsigned)N), dim3(KM_THREADS), 0, (hipStream_t)stream, X, D, k, centroids, labels,
                       (const int*)nullptr, changed);
    return status(hipGetLastError());
}

int gitcap_dbg_kmeans_update(const float* X, int N, int D, int k, const int32_t* labels, float* centroids, void* stream) {
    if (!X || !centroids || !labels || N <= 0 || D < 1 || k < 1 || k > N || k > 65535) return GITCAP_ERR_ARG;
    hipLaunchKernelGGL(kmeans_update_kernel, dim3((unsigned)((D + KM_THREADS - 1) / KM_THREADS), (unsigned)k), dim3(KM_THREADS), 0,
                       (hipStream_t)stream, X, N, D, labels, centroids, (int*)nullptr, 0, (int*)nullptr);
    return status(hipGetLastError());
}

int gitcap_frame_select(const uint8_t* keep, const int32_t* labels, int N, int max_frames, int64_t* idx, int32_t* count, void* stream) {
    if ((!keep && !labels) || !idx || !count || N <= 0 || max_frames < 1) return GITCAP_ERR_ARG;
    hipLaunchKernelGGL(frame_select_kernel, dim3(1), dim3(SEL_THREADS), 0, (hipStream_t)stream, keep, labels, N, max_frames, (long long*)idx, count);
    return status(hipGetLastError());
}

}  // extern "C"
