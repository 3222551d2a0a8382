// Per-token attention maps of the GIT decoder over frames and patches, a post-pass over the cached q and k of a text pass.
//
// For text row r (clip c = r / rows_per_clip), position j, layer l, head h:
//     p[l][h][r][j][.] = softmax over (clip c's image keys ; the row's text keys 0..j) of q . k / sqrt(64)
// -- the block mask of txt_block_kernel, on the q | k the q|k|v launch left in the text cache (q is stored unscaled) and the image
// keys of kv_img.  The outputs are means over the heads and the selected layers (all, or one):
//     frame_mass[r][j][f]  the mass on the N image tokens of frame f, 0 for f beyond the clip's frames
//     text_mass[r][j]      the mass on the row's own text keys
//     patch_map[r][j][s]   (optional) the mean probability of image token s, 0 for s beyond the clip's rows
//
// Two launches, ordered by the stream alone (no workgroup waits for another, no float atomics):
//   attn_stats_kernel  one 4-wave workgroup per (row, selected layer, head): S = Q K^T in 16 x 16 tiles (v_mfma_f32_16x16x32_bf16, q
//                      rows as the A operand, key rows as the B operand: both are 16-byte global loads of the lane's 8 consecutive
//                      columns, no LDS staging), the row maximum in a first sweep over the keys and the sum of exp2 in a second:
//                      stats [layer][head][row][position] = {max, sum} in the log2 domain.
//   attn_map_kernel    one 4-wave workgroup per (row, 16-position tile, frame of the clip | the text keys): walks its keys in
//                      chunks of 64 (one tile per wave), for every chunk the selected layers and heads in ascending order, adds
//                      exp2(s - max) / sum in registers, divides by the count, writes the patch columns and sums the chunk into the
//                      frame's mass: lane-local over the chunks in ascending order, then the 16 key lanes by a butterfly, then the
//                      four waves in wave order.
// Every sum has a fixed order that depends on (N, T) alone: a row's values do not depend on the rows beside it, and two runs
// give the same bits.  Loads are plain and clamped to a valid row (a masked lane reads the last valid key, a padded position the
// last valid position): nothing behind position T - 1 of the text cache or behind a clip's image rows is read.
#include "kernels.h"

namespace {

constexpr float kScaleLog2e = 0.125f * 1.4426950408889634f;  // 1/sqrt(64) * log2(e), as txt_block_kernel
__device__ __forceinline__ float ex2(float x) { return __builtin_amdgcn_exp2f(x); }

// one 16 (positions) x 16 (keys) tile of q . k over the 64 columns of a head: lane l holds q row (l & 15) and key row (l & 15),
// columns 8 (l >> 4) + {0, 32}; the result: key l & 15, positions 4 (l >> 4) + reg
__device__ __forceinline__ f32x4 qk_tile(const bf16_t* qp, const bf16_t* kp) {
    const bf16x8 q0 = *(const bf16x8*)qp, q1 = *(const bf16x8*)(qp + 32);
    const bf16x8 k0 = *(const bf16x8*)kp, k1 = *(const bf16x8*)(kp + 32);
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q0, k0, acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(q1, k1, acc, 0, 0, 0);
    return acc;
}

struct ClipKeys { int S; size_t row0; };
__device__ __forceinline__ ClipKeys clip_keys(const AttnMapArgs& a, int clip) {
    ClipKeys c;
    if (a.off) { c.S = min(max(a.len[clip], 0), a.Smax); c.row0 = (size_t)a.off[clip]; }
    else { c.S = a.S_img; c.row0 = (size_t)clip * a.S_img; }
    c.S = a.N > 0 ? c.S - c.S % a.N : 0;       // whole frames: the keys the statistics sum are the keys the map attributes
    return c;
}
__device__ __forceinline__ int row_len(const AttnMapArgs& a, int r) { return a.lengths ? min(max(a.lengths[r], 0), a.T) : a.T; }

__global__ __launch_bounds__(256) void attn_stats_kernel(AttnMapArgs a) {
    __shared__ float wm[4][16], ws[4][16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int nl = a.layer < 0 ? a.L : 1;
    const int head = blockIdx.x % a.H, lsel = (blockIdx.x / a.H) % nl, r = blockIdx.x / (a.H * nl);
    const int layer = a.layer < 0 ? lsel : a.layer;
    const int ld = 3 * a.D, key_l = lane & 15, fq = lane >> 4;
    const ClipKeys ck = clip_keys(a, r / a.rows_per_clip);
    const int len_r = row_len(a, r);
    const bf16_t* txt = a.kv_txt + (size_t)layer * a.txt_layer_stride + (size_t)r * a.Tmax * ld + head * 64 + fq * 8;
    const bf16_t* img = a.kv_img + (size_t)layer * a.img_layer_stride + ck.row0 * ld + a.D + head * 64 + fq * 8;
    const int img_tiles = (ck.S + 15) >> 4;
    float* st = a.stats + ((size_t)(lsel * a.H + head) * a.rows + r) * a.T * 2;

    for (int pos0 = 0; pos0 < len_r; pos0 += 16) {
        const bf16_t* qp = txt + (size_t)min(pos0 + key_l, a.T - 1) * ld;
        const int ntiles = img_tiles + (pos0 >> 4) + 1;
        int posc[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) posc[i] = min(pos0 + fq * 4 + i, a.T - 1);
        // the scores of tile i in the log2 domain, -inf where the lane's key does not exist for the position
        auto tile = [&](int i, float (&t)[4]) {
            const bool image = i < img_tiles;
            const int key = (image ? i : i - img_tiles) * 16 + key_l;
            const bf16_t* kp = image ? img + (size_t)min(key, ck.S - 1) * ld : txt + a.D + (size_t)min(key, a.T - 1) * ld;
            const f32x4 s = qk_tile(qp, kp);
#pragma unroll
            for (int u = 0; u < 4; ++u) t[u] = (image ? key < ck.S : key <= posc[u]) ? s[u] * kScaleLog2e : -INFINITY;
        };
        float m[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
        for (int i = wid; i < ntiles; i += 4) {
            float t[4];
            tile(i, t);
#pragma unroll
            for (int u = 0; u < 4; ++u) m[u] = fmaxf(m[u], t[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) m[u] = fmaxf(m[u], __shfl_xor(m[u], o));
            if (key_l == 0) wm[wid][fq * 4 + u] = m[u];
        }
        __syncthreads();
        // (text key 0 exists for every position, so the maximum over the four waves is finite)
#pragma unroll
        for (int u = 0; u < 4; ++u) m[u] = fmaxf(fmaxf(wm[0][fq * 4 + u], wm[1][fq * 4 + u]), fmaxf(wm[2][fq * 4 + u], wm[3][fq * 4 + u]));
        float l[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = wid; i < ntiles; i += 4) {
            float t[4];
            tile(i, t);
#pragma unroll
            for (int u = 0; u < 4; ++u) l[u] += ex2(t[u] - m[u]);
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
#pragma unroll
            for (int o = 1; o < 16; o <<= 1) l[u] += __shfl_xor(l[u], o);
            if (key_l == 0) ws[wid][fq * 4 + u] = l[u];
        }
        __syncthreads();
        if (tid < 16 && pos0 + tid < a.T) {
            const float sum = ((ws[0][tid] + ws[1][tid]) + ws[2][tid]) + ws[3][tid];
            const float mx = fmaxf(fmaxf(wm[0][tid], wm[1][tid]), fmaxf(wm[2][tid], wm[3][tid]));
            *(float2*)(st + (size_t)(pos0 + tid) * 2) = make_float2(mx, sum);
        }
        __syncthreads();        // wm and ws are read above: the next position tile's waves must not store over them yet
    }
}

__global__ __launch_bounds__(256) void attn_map_kernel(AttnMapArgs a) {
    __shared__ float red[4][16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Fmax = a.N > 0 ? a.Smax / a.N : 0, PT = (a.T + 15) >> 4;
    const int f = blockIdx.x % (Fmax + 1), pt = (blockIdx.x / (Fmax + 1)) % PT, r = blockIdx.x / ((Fmax + 1) * PT);
    const bool text = f == Fmax;
    const int nl = a.layer < 0 ? a.L : 1;
    const int ld = 3 * a.D, key_l = lane & 15, fq = lane >> 4, pos0 = pt * 16;
    const ClipKeys ck = clip_keys(a, r / a.rows_per_clip);
    const int len_r = row_len(a, r);
    const int Fc = a.N > 0 ? ck.S / a.N : 0;
    float* const fm_out = text ? a.text_mass + (size_t)r * a.T : a.frame_mass + (size_t)r * a.T * a.ld_f + f;
    const int fm_ld = text ? 1 : a.ld_f;

    if (pos0 >= len_r || (!text && f >= Fc)) {      // nothing to compute: the tile's outputs are exact zeros
        if (tid < 16 && pos0 + tid < a.T) fm_out[(size_t)(pos0 + tid) * fm_ld] = 0.f;
        if (!text && a.patch_map)
            for (int e = tid; e < 16 * a.N; e += 256) {
                const int p = pos0 + e / a.N;
                if (p < a.T) a.patch_map[((size_t)r * a.T + p) * a.ld_s + (size_t)f * a.N + e % a.N] = 0.f;
            }
        return;
    }
    const int nk = text ? min(pos0 + 16, a.T) : a.N;                    // keys of this workgroup (text: causal, masked per position)
    const size_t txt_row = (size_t)r * a.Tmax * ld;
    const size_t q_off = txt_row + (size_t)min(pos0 + key_l, a.T - 1) * ld + fq * 8;
    const size_t key_row0 = text ? txt_row + a.D : (ck.row0 + (size_t)f * a.N) * ld + a.D;
    const bf16_t* const kbase = text ? a.kv_txt : a.kv_img;
    const size_t klayer = text ? a.txt_layer_stride : a.img_layer_stride;
    int pos[4], posc[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) { pos[u] = pos0 + fq * 4 + u; posc[u] = min(pos[u], a.T - 1); }
    const float cnt = (float)(nl * a.H);

    float fm[4] = {0.f, 0.f, 0.f, 0.f};
    for (int c0 = wid * 16; c0 < nk; c0 += 64) {                        // wave-uniform: the wave's tile of this chunk of 64 keys
        const int key = c0 + key_l;
        const size_t k_off = key_row0 + (size_t)min(key, nk - 1) * ld + fq * 8;
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int lsel = 0; lsel < nl; ++lsel) {
            const int layer = a.layer < 0 ? lsel : a.layer;
            const bf16_t* qp = a.kv_txt + (size_t)layer * a.txt_layer_stride + q_off;
            const bf16_t* kp = kbase + (size_t)layer * klayer + k_off;
            for (int h = 0; h < a.H; ++h) {
                const f32x4 s = qk_tile(qp + h * 64, kp + h * 64);
                const float* st = a.stats + ((size_t)(lsel * a.H + h) * a.rows + r) * a.T * 2;
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float2 ms = *(const float2*)(st + (size_t)posc[u] * 2);
                    const float p = ex2(s[u] * kScaleLog2e - ms.x) / ms.y;
                    const bool valid = key < nk && (!text || key <= pos[u]) && pos[u] < len_r;
                    acc[u] += valid ? p : 0.f;
                }
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            acc[u] = acc[u] / cnt;
            if (!text && a.patch_map && key < nk && pos[u] < a.T)
                a.patch_map[((size_t)r * a.T + pos[u]) * a.ld_s + (size_t)f * a.N + key] = acc[u];
            fm[u] += acc[u];
        }
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) fm[u] += __shfl_xor(fm[u], o);
        if (key_l == 0) red[wid][fq * 4 + u] = fm[u];
    }
    __syncthreads();
    if (tid < 16 && pos0 + tid < a.T) fm_out[(size_t)(pos0 + tid) * fm_ld] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

}  // namespace

size_t attn_map_scratch_floats(int L, int H, int rows, int T, int layer) { return (size_t)(layer < 0 ? L : 1) * H * rows * T * 2; }

hipError_t launch_attn_map(const AttnMapArgs& a, hipStream_t s) {
    if (!a.kv_txt || !a.stats || !a.frame_mass || !a.text_mass) return hipErrorInvalidValue;
    if (a.L <= 0 || a.H <= 0 || a.D != a.H * 64 || a.rows <= 0 || a.rows_per_clip <= 0 || a.rows % a.rows_per_clip != 0) return hipErrorInvalidValue;
    if (a.T <= 0 || a.T > a.Tmax || a.layer < -1 || a.layer >= a.L) return hipErrorInvalidValue;
    if (a.N < 0 || a.Smax < 0 || (a.N == 0 ? a.Smax != 0 : a.Smax % a.N != 0)) return hipErrorInvalidValue;
    if ((a.off == nullptr) != (a.len == nullptr)) return hipErrorInvalidValue;
    if (!a.off && a.S_img != a.Smax) return hipErrorInvalidValue;
    if (a.Smax > 0 && !a.kv_img) return hipErrorInvalidValue;
    const int Fmax = a.N > 0 ? a.Smax / a.N : 0;
    if (a.ld_f < Fmax || (a.patch_map && a.ld_s < a.Smax)) return hipErrorInvalidValue;
    if (((uintptr_t)a.kv_txt & 15) != 0 || ((uintptr_t)a.kv_img & 15) != 0 || ((uintptr_t)a.stats & 7) != 0) return hipErrorInvalidValue;
    const int nl = a.layer < 0 ? a.L : 1, PT = (a.T + 15) / 16;
    const long long g1 = (long long)a.rows * nl * a.H, g2 = (long long)a.rows * PT * (Fmax + 1);
    if (g1 > 0x7fffffffLL || g2 > 0x7fffffffLL) return hipErrorInvalidValue;
    attn_stats_kernel<<<dim3((unsigned)g1), dim3(256), 0, s>>>(a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    attn_map_kernel<<<dim3((unsigned)g2), dim3(256), 0, s>>>(a);
    return hipGetLastError();
}
