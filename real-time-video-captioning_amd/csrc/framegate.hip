// Scene-change distances of pushed camera frames (include/gitcap.h: gitcap_frame_change), the device side of gitcap.framegate.
// Replaces the arithmetic of the reference's frame samplers (src/utils/frame_sampling_methods.py:201-297): the mean squared error
// of a frame against the last frame kept, and the chi-square distance of their 256-bin histograms of one channel.
//
// One pass over both frames (frame_change_kernel) gives three integer results per clip -- the sum of squared byte differences and
// the two histograms -- and a one-wave finalize turns them into the two fp64 distances.  Everything up to the finalize is integer
// arithmetic, so the results do not depend on the order of the reduction:
//   * a thread owns 48 consecutive bytes of both frames (three 16-byte loads each).  48 is a multiple of 3, so which bytes of a chunk
//     belong to the wanted channel is the same pattern for every chunk of a frame (SEL, a template parameter);
//   * (a - b)^2 = a^2 + b^2 - 2ab: three packed 4 x 8-bit dot products per dword, exact in 32 bits (one chunk stays below 2^23);
//     chunks are added up in 64 bits per thread;
//   * histograms are private to a wave in LDS (integer LDS atomics: a frame of one colour sends all 64 lanes to one counter, which
//     the LDS serialises -- slower, still exact), merged once per workgroup and folded into the call's scratch with 32-bit vector
//     atomics; the sum of squares with one 64-bit atomic per workgroup;
//   * bytes in front of the first 16-byte boundary and behind the last whole chunk are taken one at a time (any H x W, any frame
//     offset); a pair of frames whose addresses differ modulo 16 is taken one byte at a time altogether.
// The scratch (8 + 2 KB per clip) is a stream-ordered allocation of the call, zeroed on the call's stream: no state outlives a call
// and two calls on two streams share nothing.
#include "../../include/gitcap.h"
#include "kernels.h"

namespace {

constexpr int FC_THREADS = 256, FC_WAVES = FC_THREADS / 64;
constexpr int FC_CHUNK = 48;                 // bytes per thread and step: three 16-byte loads, a whole number of BGR triples
constexpr int FC_CHUNKS_PER_THREAD = 4;      // the launcher sizes the grid for about this many steps per thread
constexpr int FC_MAX_BLOCKS = 256;           // workgroups per clip at most (larger frames: more steps per thread)

// scratch of one call: ssd[B] (64-bit), then hist[B][2][256] (0 = frame, 1 = ref)
__host__ __device__ inline size_t fc_hist_offset(int B) { return (size_t)B * sizeof(unsigned long long); }
inline size_t fc_scratch_bytes(int B) { return fc_hist_offset(B) + (size_t)B * 2 * 256 * sizeof(unsigned); }

// sum of the squared byte differences of two dwords
__device__ __forceinline__ unsigned sq_diff4(unsigned a, unsigned b) {
    const unsigned aa = __builtin_amdgcn_udot4(a, a, 0u, false), bb = __builtin_amdgcn_udot4(b, b, 0u, false);
    return aa + bb - 2u * __builtin_amdgcn_udot4(a, b, 0u, false);
}

// One chunk.  SEL = index modulo 3, within the chunk, of the bytes of the wanted channel.
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

// grid (workgroups per clip, B).  N = H*W*3 bytes per frame; scratch as fc_scratch_bytes lays it out, zero on entry.
__global__ __launch_bounds__(FC_THREADS) void frame_change_kernel(const unsigned char* __restrict__ frames, const unsigned char* __restrict__ ref,
                                                                  int64_t N, int channel, int B, unsigned char* __restrict__ scratch) {
    __shared__ unsigned hist[FC_WAVES][2][256];
    __shared__ unsigned long long blk_ssd;
    const int tid = threadIdx.x, wave = tid >> 6, b = blockIdx.y;
    for (int i = tid; i < FC_WAVES * 2 * 256; i += FC_THREADS) (&hist[0][0][0])[i] = 0u;
    if (tid == 0) blk_ssd = 0ull;
    __syncthreads();
    unsigned* hf = hist[wave][0];
    unsigned* hr = hist[wave][1];

    const unsigned char* f = frames + (int64_t)b * N;
    const unsigned char* r = ref + (int64_t)b * N;
    // [0, head): bytes in front of the frame's first 16-byte boundary; then `chunks` whole chunks; the rest one at a time again.
    // The reference frame must reach its boundary with the same head, else there are no chunks at all.
    int64_t head = (int64_t)((16u - (unsigned)((uintptr_t)f & 15u)) & 15u);
    if (head > N) head = N;
    int64_t chunks = (N - head) / FC_CHUNK;
    if (((uintptr_t)(r + head) & 15u) != 0) { head = 0; chunks = 0; }
    const int64_t body = chunks * FC_CHUNK;

    unsigned long long s = 0;
    // byte k of a chunk is byte head + k (mod 3) of a BGR triple (frames start on a triple: N is a multiple of 3)
    switch ((channel + 3 - (int)(head % 3)) % 3) {
        case 0: s = fc_body<0>(f + head, r + head, chunks, hf, hr); break;
        case 1: s = fc_body<1>(f + head, r + head, chunks, hf, hr); break;
        default: s = fc_body<2>(f + head, r + head, chunks, hf, hr); break;
    }
    for (int64_t i = (int64_t)blockIdx.x * FC_THREADS + tid; i < N - body; i += (int64_t)gridDim.x * FC_THREADS) {
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
    unsigned long long* ssd = (unsigned long long*)scratch;
    unsigned* gh = (unsigned*)(scratch + fc_hist_offset(B)) + (size_t)b * 512;
    if (tid == 0) atomicAdd(&ssd[b], blk_ssd);
#pragma unroll
    for (int k = 0; k < 2; ++k) {                          // thread = bin
        unsigned n = 0;
#pragma unroll
        for (int w = 0; w < FC_WAVES; ++w) n += hist[w][k][tid];
        if (n) atomicAdd(&gh[k * 256 + tid], n);
    }
}

// grid B, one wave: copies the integer results out and writes the two distances.  chi-square: the 256 terms are computed four per
// lane, then lane 0 adds them in ascending bin order (a bin the reference frame does not have contributes +0.0, which leaves the
// fp64 sum as it is), so the result has one defined operation order.
__global__ __launch_bounds__(64) void frame_change_finalize_kernel(const unsigned char* __restrict__ scratch, int B, int64_t N,
                                                                   unsigned long long* __restrict__ ssd_out, unsigned* __restrict__ hist_frame,
                                                                   unsigned* __restrict__ hist_ref, double* __restrict__ mse,
                                                                   double* __restrict__ chisq) {
    __shared__ double term[256];
    const int b = blockIdx.x, lane = threadIdx.x;
    const unsigned long long* ssd = (const unsigned long long*)scratch;
    const unsigned* gh = (const unsigned*)(scratch + fc_hist_offset(B)) + (size_t)b * 512;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int i = lane + 64 * k;
        const unsigned nf = gh[i], nr = gh[256 + i];
        if (hist_frame) hist_frame[(size_t)b * 256 + i] = nf;
        if (hist_ref) hist_ref[(size_t)b * 256 + i] = nr;
        const long long d = (long long)nr - (long long)nf;
        term[i] = nr ? (double)(d * d) / (double)nr : 0.0;
    }
    __syncthreads();
    if (lane == 0) {
        const unsigned long long s = ssd[b];
        if (ssd_out) ssd_out[b] = s;
        if (mse) mse[b] = (double)s / (double)N;
        if (chisq) {
            double acc = 0.0;
            for (int i = 0; i < 256; ++i) acc += term[i];
            chisq[b] = acc;
        }
    }
}

}  // namespace

extern "C" {

int gitcap_frame_change(const uint8_t* frames_hwc_bgr, const uint8_t* ref_hwc_bgr, int B, int H, int W, int channel,
                        uint64_t* ssd, uint32_t* hist_frame, uint32_t* hist_ref, double* mse, double* chisq, void* stream) {
    if (!frames_hwc_bgr || !ref_hwc_bgr || B < 1 || H < 1 || W < 1 || channel < 0 || channel > 2) return GITCAP_ERR_ARG;
    const int64_t N = (int64_t)H * W * 3;
    if (N > INT32_MAX || B > 65535) return GITCAP_ERR_ARG;          // 32-bit bin counts; grid.y
    if (!ssd && !hist_frame && !hist_ref && !mse && !chisq) return 0;
    hipStream_t s = (hipStream_t)stream;
    void* scratch = nullptr;
    if (hipMallocAsync(&scratch, fc_scratch_bytes(B), s) != hipSuccess) return GITCAP_ERR_NOMEM;
    hipError_t e = hipMemsetAsync(scratch, 0, fc_scratch_bytes(B), s);
    if (e == hipSuccess) {
        const int64_t per_block = (int64_t)FC_THREADS * FC_CHUNK * FC_CHUNKS_PER_THREAD;
        int64_t blocks = (N + per_block - 1) / per_block;
        if (blocks > FC_MAX_BLOCKS) blocks = FC_MAX_BLOCKS;
        hipLaunchKernelGGL(frame_change_kernel, dim3((unsigned)blocks, (unsigned)B), dim3(FC_THREADS), 0, s, frames_hwc_bgr, ref_hwc_bgr, N,
                           channel, B, (unsigned char*)scratch);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        hipLaunchKernelGGL(frame_change_finalize_kernel, dim3((unsigned)B), dim3(64), 0, s, (const unsigned char*)scratch, B, N,
                           (unsigned long long*)ssd, hist_frame, hist_ref, mse, chisq);
        e = hipGetLastError();
    }
    (void)hipFreeAsync(scratch, s);
    return e == hipSuccess ? 0 : GITCAP_ERR_HIP;
}

}  // extern "C"
