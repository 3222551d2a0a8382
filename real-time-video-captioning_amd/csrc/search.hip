// Candidate generation of the search loops and the device-resident beam state: beam top-k, sampled draws, the ban mask of
// constrained decoding, and the beam bookkeeping (step, finish, init).  Topic by topic: the kernels, then their launchers.
#include "kernels.h"
#include <algorithm>
#include <cmath>
#include "prompt_sel.h"

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
namespace {
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
}  // namespace
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
namespace {
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
}  // namespace
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

// ---- ban mask of constrained decoding (gitcap_attach_constraints; kernels.h: launch_ban_mask) -------------------------------------
// One workgroup per row.  The row's bitmap is built in LDS (32-bit words, V <= 131072: 16 KB) -- cleared, a barrier, the three rules
// set their bits with LDS atomics, a barrier -- and then EVERY 32-bit word of the row's ld_mask / 2 is stored, the ones behind
// ceil(V / 16) as 0: the result does not depend on what the buffer held (it is reused every step) and needs no global atomic.
// A uint16 word c >> 4, bit c & 15 of the mask is bit c & 31 of 32-bit word c >> 5 (little endian): the same bytes.
//   n-gram (n >= 1; HF NoRepeatNGramLogitsProcessor): thread i <= cur_len - n compares prefix[i .. i + n - 2] with the last n - 1
//           tokens prefix[cur_len - n + 1 .. cur_len - 1] as int64 values and bans prefix[i + n - 1]; nothing while cur_len < n;
//   length: sep_id while cur_len < min_length (HF MinLengthLogitsProcessor);   suppress: the listed ids.
// An id outside [0, V) sets no bit, so the bits of the last word beyond V stay 0.
// The rules (n, min_length, the suppress list) reach the body from the launch (BanRulesArgs: kernel arguments, the teacher's loops) or
// from a device record read when the kernel runs (BanRulesRec; kernels.h: launch_ban_mask_rec), so that a captured token loop
// follows whatever record was written last.  The record's list length is clamped to the record, so no value in it reads past it.
namespace {
constexpr int BM_MAX_V = 131072;

struct BanRules { int n, min_length; const int32_t* suppress; int n_suppress; };
struct BanRulesArgs {
    int n, min_length; const int32_t* suppress; int n_suppress;
    __device__ __forceinline__ BanRules load() const { return BanRules{n, min_length, suppress, n_suppress}; }
};
struct BanRulesRec {
    const int32_t* rec;     // int32 [BAN_REC_WORDS]: n, min_length, n_suppress, 0, the ids
    __device__ __forceinline__ BanRules load() const {
        return BanRules{rec[0], rec[1], rec + BAN_REC_HEADER, min(max(rec[2], 0), BAN_REC_MAX_SUPPRESS)};
    }
};

template <typename Rules>
__device__ __forceinline__ void ban_mask_body(const int64_t* __restrict__ ids, int ld_ids, int cur_len, const Rules rules, int sep_id, int V,
                                              unsigned* __restrict__ mask32, int ld32) {
    __shared__ unsigned bits[BM_MAX_V / 32];
    const BanRules ru = rules.load();
    const int n = ru.n, min_length = ru.min_length, n_suppress = ru.n_suppress;
    const int32_t* __restrict__ suppress = ru.suppress;
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

__global__ __launch_bounds__(256) void ban_mask_kernel(const int64_t* __restrict__ ids, int ld_ids, int cur_len, int n, int min_length,
                                                       int sep_id, const int32_t* __restrict__ suppress, int n_suppress, int V,
                                                       unsigned* __restrict__ mask32, int ld32) {
    ban_mask_body(ids, ld_ids, cur_len, BanRulesArgs{n, min_length, suppress, n_suppress}, sep_id, V, mask32, ld32);
}
__global__ __launch_bounds__(256) void ban_mask_rec_kernel(const int64_t* __restrict__ ids, int ld_ids, int cur_len, int sep_id,
                                                           const int32_t* __restrict__ rec, int V, unsigned* __restrict__ mask32, int ld32) {
    ban_mask_body(ids, ld_ids, cur_len, BanRulesRec{rec}, sep_id, V, mask32, ld32);
}

bool ban_mask_args_ok(const int64_t* ids, int ld_ids, int rows, int cur_len, int V, const uint16_t* mask, int ld_mask) {
    return ids && mask && rows > 0 && cur_len >= 0 && ld_ids >= cur_len && V > 0 && V <= BM_MAX_V && ld_mask >= (V + 15) / 16 && !(ld_mask & 1) &&
           !((uintptr_t)mask & 3);
}
}  // namespace
hipError_t launch_ban_mask(const int64_t* ids, int ld_ids, int rows, int cur_len, int n, int min_length, int sep_id,
                           const int32_t* suppress, int n_suppress, int V, uint16_t* mask, int ld_mask, hipStream_t s) {
    if (!ban_mask_args_ok(ids, ld_ids, rows, cur_len, V, mask, ld_mask) || n < 0 || min_length < 0 || n_suppress < 0 ||
        n_suppress > BAN_REC_MAX_SUPPRESS || (n_suppress > 0 && !suppress))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(ban_mask_kernel, dim3(rows), dim3(256), 0, s, ids, ld_ids, cur_len, n, min_length, sep_id, suppress, n_suppress, V,
                       (unsigned*)mask, ld_mask / 2);
    return hipGetLastError();
}
hipError_t launch_ban_mask_rec(const int64_t* ids, int ld_ids, int rows, int cur_len, int sep_id, const int32_t* rec, int V, uint16_t* mask,
                               int ld_mask, hipStream_t s) {
    if (!ban_mask_args_ok(ids, ld_ids, rows, cur_len, V, mask, ld_mask) || !rec || ((uintptr_t)rec & 3)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ban_mask_rec_kernel, dim3(rows), dim3(256), 0, s, ids, ld_ids, cur_len, sep_id, rec, V, (unsigned*)mask, ld_mask / 2);
    return hipGetLastError();
}

// ---- device-side beam bookkeeping: one step of GeneratorWithBeamSearchV2.search (model.py:573-621) -----
// One block per batch element; thread 0 walks the <= 16 sorted candidates exactly like the reference's
// Python loop (finished hypotheses kept n_best = 1: score = sum_logprob / len^length_penalty, :503, :592-594;
// is_done test :576), then the block copies the surviving prefixes into the next id buffer (:620-621).
namespace {
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
}  // namespace
static BeamState beam_state(const BeamBuffers& bb) {
    return BeamState{{bb.ids0, bb.ids1}, bb.beam_scores, bb.words, bb.src_rows, bb.done, bb.hyp_len, bb.hyp_score, bb.hyp_ids};
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

// decoded[b][k] = the stored hypothesis of rank k by descending score (equal scores in storage order) + EOS padding, logprobs[b][k]
// = its score; a rank with no hypothesis is all-EOS with score -1e5 (model.py:653-678).  One workgroup per (clip, slot): it counts
// the slots ranked before its own.  first_decoded / first_logprobs: rank 0 once more, [B][max_len] / [B].  Every output is nullable.
namespace {
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
}  // namespace
hipError_t launch_beam_finish(const BeamBuffers& bb, int n, int B, int max_len, int eos, const BeamFinishOut& o, hipStream_t s) {
    if (n < 1 || n > 16) return hipErrorInvalidValue;
    hipLaunchKernelGGL(beam_finish_kernel, dim3(B, n), dim3(64), 0, s, beam_state(bb), n, max_len, eos, o.decoded, o.logprobs, o.first_decoded,
                       o.first_logprobs);
    return hipGetLastError();
}

hipError_t launch_beam_init(const BeamBuffers& bb, int B, int beams, int n, int max_len, int cls, hipStream_t s) {
    if (n < 1 || n > 16) return hipErrorInvalidValue;
    hipLaunchKernelGGL(beam_init_kernel, dim3((B * std::max(beams, n) + 63) / 64), dim3(64), 0, s, beam_state(bb), B, beams, n, max_len, cls);
    return hipGetLastError();
}
