// Skinny GEMMs for the text path (M = rows*T is a handful of 16-row tiles):
//     out[m][n] = X[m][:] . W[n][:]
// HBM/latency bound weight streaming, not MFMA bound.  Every weight element is read exactly once,
// straight from HBM into VGPRs (no LDS round trip: a weight tile is not shared between waves;
// cdna_hip_programming.md "GEMV / M <= 16 decode weights").  The 16x16x32 bf16 MFMA is used because
// 16 activation rows fit its N dimension exactly, so the dot products cost no VALU.
//
// One wave (= one 64-thread block, to spread over as many CUs as possible) owns one 16-row weight
// tile; all of its weight fragments are requested back-to-back before the first MFMA so that a
// whole matrix is in flight at once (a 768x768 matrix is 1.2 MB = 48 waves x 24 KiB).
//
//   skinny_full  : whole K per wave, fused epilogue (bias [+GELU] -> bf16, or fp32 logits + a
//                  per-tile arg-max partial for the vocabulary head).
//   skinny_head  : the vocabulary head (SK_BIAS_F32 over many tiles): four tiles per workgroup share the activation m-tile
//                  through LDS instead of fetching it once per tile (round 4; same MFMA chain, same bits).
//   skinny_rows3 : the row-prologue form over the fused FFN's 48 slabs: three waves share the slab reduce (round 4).
//   skinny_splitk: K split over blocks (more waves in flight for the K=3072 matrix and for the
//                  N=768 ones that would otherwise use 48 waves); each wave writes its fp32
//                  partial tile to a slab; ln_reduce_kernel (select.hip) sums the slabs in a fixed
//                  order, adds bias + residual and applies LayerNorm.  No atomics: results are
//                  bitwise reproducible and independent of the batch size.
//
// Row prologue (LNR, one or two text rows: the single-clip case): the token loop is a chain of dependent launches of
// ~5 us each, and with one row the launch that only normalises it costs as much as one that streams a matrix.  With
// LNR every workgroup of the q|k|v launch computes the row(s) itself (rowln.h: the code of the stand-alone kernels, so
// the same bits) right after requesting its weight fragments -- the two latencies overlap -- and keeps them in LDS;
// 24 KB of slabs per row, read by 144 workgroups through L2, is nothing.  (For more rows the redundant reads and the
// serial row loop cost more than the launch.)
#include "kernels.h"
#include "rowln.h"
#include "lp_partials.h"

namespace {

// weight fragments of one 16-row tile, K32 k-steps.  FP8: e4m3 bytes (8 per lane and k-step, half the stream),
// expanded in registers to bf16 times the row's power-of-two scale (exact: the bf16-stored weight bit for bit).
// Wpk != nullptr: the fragment-major copy (launch_pack_frags): fragment k of this wave = 1 KiB (512 B) contiguous per
// wave instruction, `kofs` / 32 k-steps into tile `row` / 16 -- 3-4 x the per-CU pull rate of the row-major pattern.
template <int K32, bool FP8>
__device__ __forceinline__ void load_wfrags(const void* W, const void* Wpk, const float* wscale, size_t row, int K, int kofs, bf16x8 (&wf)[K32]) {
    if (Wpk) {
        const int lane = threadIdx.x & 63;
        const size_t f0 = ((row >> 4) * (size_t)(K >> 5) + (size_t)(kofs >> 5)) * 64 + lane;      // fragment index of k-step 0
        if (FP8) {
            const uint2* wp = (const uint2*)Wpk + f0;
            const float sc = wscale[row];
            uint2 raw[K32];
#pragma unroll
            for (int k = 0; k < K32; ++k) raw[k] = wp[(size_t)k * 64];
#pragma unroll
            for (int k = 0; k < K32; ++k) wf[k] = fp8x8_to_bf16x8(raw[k], sc);
        } else {
            const bf16x8* wp = (const bf16x8*)Wpk + f0;
#pragma unroll
            for (int k = 0; k < K32; ++k) wf[k] = wp[(size_t)k * 64];
        }
        return;
    }
    if (FP8) {
        const unsigned char* wp = (const unsigned char*)W + row * K + kofs;
        const float sc = wscale[row];
        uint2 raw[K32];
#pragma unroll
        for (int k = 0; k < K32; ++k) raw[k] = *(const uint2*)(wp + k * 32);
#pragma unroll
        for (int k = 0; k < K32; ++k) wf[k] = fp8x8_to_bf16x8(raw[k], sc);
    } else {
        const bf16_t* wp = (const bf16_t*)W + row * K + kofs;
#pragma unroll
        for (int k = 0; k < K32; ++k) wf[k] = *(const bf16x8*)(wp + k * 32);
    }
}

// the given next token of head row m (kernels.h: HeadTargets), -1 where the row has none
__device__ __forceinline__ int64_t head_target(const HeadTargets& t, const int m) {
    const int r = m / t.T, j = m - r * t.T + t.shift;
    return j < t.T ? t.ids[(size_t)r * t.ld + j] : -1;
}

// fp32 logits of one 16 x 16 tile (lane: out[m][n .. n+3]) and the tile's arg-max partial per row (ascending n: first max wins)
// LSE: also the tile's third partial (a.amax_sum) -- kernels of their own, picked by the launcher where the pointer is set, so that
// the launches without it stay the code they were
// TGT (the scoring head, with LSE): the lane that holds column tcol of row m -- the row's given next token -- also stores that logit
// to tlogit[m]; a column outside [0, N) is in no lane.  Padded rows and idle waves (!mvalid) store nothing.
template <bool LSE, bool TGT = false>
__device__ __forceinline__ void logits_epilogue(const SkinnyArgs& a, const float (&y)[4], const int m, const bool mvalid, const int n,
                                                const int fq, const int tile, const int ntiles, const int64_t tcol = -1,
                                                float* tlogit = nullptr) {
    if (TGT) {
        if (mvalid && tcol >= n && tcol < n + 4 && tcol < a.N) {
#pragma unroll
            for (int r = 0; r < 4; ++r)                         // (one store each: an indexed pick of y[] would move it out of registers)
                if (tcol == n + r) tlogit[m] = y[r];
        }
    }
    if (mvalid && a.out) {
        float* op = (float*)a.out + (size_t)m * a.ldo + n;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (n + r < a.N) op[r] = y[r];
    }
    if (a.amax_val) {
        float best = -INFINITY;
        int bi = 0x7fffffff;
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (n + r < a.N && (y[r] > best)) { best = y[r]; bi = n + r; }
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) {
            const float v2 = __shfl_xor(best, off);
            const int i2 = __shfl_xor(bi, off);
            if (v2 > best || (v2 == best && i2 < bi)) { best = v2; bi = i2; }
        }
        if (fq == 0 && mvalid) {
            a.amax_val[(size_t)m * ntiles + tile] = best;
            a.amax_idx[(size_t)m * ntiles + tile] = bi;
        }
        // third partial (token log-probabilities attached): sum of exp(logit - tile max) over the tile's valid columns, the lane's
        // own columns in ascending order, then the four column groups by the butterfly above; 0 for a tile with no logit above -inf
        // (never -inf - -inf).  argmax_final / draft_accept (select.hip) merge the tiles in a fixed order.
        if (LSE) {
            float se = 0.f;
            if (best != -INFINITY) {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n + r < a.N) se += __expf(y[r] - best);
            }
#pragma unroll
            for (int off = 16; off < 64; off <<= 1) se += __shfl_xor(se, off);
            if (fq == 0 && mvalid) a.amax_sum[(size_t)m * ntiles + tile] = se;
        }
    }
}

template <int K32, int EPI, bool FP8, bool LNR, bool LSE = false>
__global__ __launch_bounds__(64) void skinny_full_kernel(SkinnyArgs a) {
    const int lane = threadIdx.x;
    const int frow = lane & 15, fq = lane >> 4;
    const int n0 = blockIdx.x * 16;
    bf16x8 wf[K32];
    load_wfrags<K32, FP8>(a.W, a.Wpk, a.wscale, (size_t)(n0 + frow), a.K, fq * 8, wf);
    __shared__ __attribute__((aligned(16))) bf16_t xrow[LNR ? 2 : 1][LNR ? K32 * 32 : 8];
    if (LNR) {
        constexpr int NV = (K32 * 32 + 255) / 256;
        const SkinnyArgs::RowPrologue& p = a.ln;
        for (int m = 0; m < a.M; ++m) {
            f32x4 v[NV], gv[NV], bev[NV];
            row_load_vec<NV>(gv, p.g, a.K, lane);                // gamma / beta: requested ahead of the row's own loads
            row_load_vec<NV>(bev, p.b, a.K, lane);
            const float s = p.kind == 1 ? row_load_reduce<NV>(v, p.slabs, p.nslab, p.bias, p.resid, a.M, a.K, m, lane)
                                        : row_load_embed<NV>(v, p.ids, p.ld_ids, p.T, p.t0, p.word, p.pos, a.K, p.vocab, m, lane);
            row_layernorm_v<NV>(v, s, lane, a.K, p.eps, gv, bev);
            row_store<NV>(v, lane, a.K, blockIdx.x == 0 ? p.xf + (size_t)m * a.K : nullptr, (bf16_t*)nullptr);
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = i * 256 + lane * 4;
                if (c < K32 * 32) {
                    uint2 o;
                    o.x = pack_bf2(v[i][0], v[i][1]);
                    o.y = pack_bf2(v[i][2], v[i][3]);
                    *(uint2*)(&xrow[m][c]) = o;
                }
            }
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_wave_barrier();
    }

    const int n = n0 + fq * 4;
    float bias[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[r] = (a.bias && n + r < a.N) ? a.bias[n + r] : 0.f;

    const int mtiles = (a.M + 15) >> 4;
    // the activation fragments of m-tile mt + 1 are requested before the MFMAs of m-tile mt (32 or more rows: a second
    // m-tile used to add a whole load -> MFMA -> store round trip to the launch)
    bf16x8 xnext[LNR ? 1 : K32];
    auto load_x = [&](int mt) {
        if (LNR) return;
        int m = mt * 16 + frow;
        m = m < a.M ? m : a.M - 1;
        const bf16_t* xp = a.X + (size_t)m * a.ldx + fq * 8;
#pragma unroll
        for (int k = 0; k < K32; ++k) xnext[LNR ? 0 : k] = *(const bf16x8*)(xp + k * 32);
    };
    load_x(0);
    for (int mt = 0; mt < mtiles; ++mt) {
        int m = mt * 16 + frow;
        const bool mvalid = m < a.M;
        m = mvalid ? m : a.M - 1;                               // clamp: padded rows are discarded
        bf16x8 xcur[LNR ? 1 : K32];
        if (!LNR) {
#pragma unroll
            for (int k = 0; k < K32; ++k) xcur[k] = xnext[k];
            if (mt + 1 < mtiles) load_x(mt + 1);
        }
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < K32; ++k) {
            const bf16x8 xf = LNR ? *(const bf16x8*)(&xrow[m][fq * 8 + k * 32]) : xcur[LNR ? 0 : k];
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[k], xf, acc, 0, 0, 0);
        }
        // lane holds out[m][n .. n+3]
        float y[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] = acc[r] + bias[r];
        if (EPI == SK_BIAS_GELU_BF16) {
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = erf_gelu(y[r]);
        } else if (EPI == SK_BIAS_RELU_BF16) {
#pragma unroll
            for (int r = 0; r < 4; ++r) y[r] = fmaxf(y[r], 0.f);
        }
        if (EPI == SK_BIAS_BF16 || EPI == SK_BIAS_GELU_BF16 || EPI == SK_BIAS_RELU_BF16) {
            if (mvalid) {
                const int orow = (m / a.T) * a.row_stride + a.row_off + (m % a.T);
                bf16_t* op = (bf16_t*)a.out + (size_t)orow * a.ldo + n;
                if (n + 3 < a.N) {
                    uint2 v;
                    v.x = pack_bf2(y[0], y[1]);
                    v.y = pack_bf2(y[2], y[3]);
                    *(uint2*)op = v;
                } else {
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (n + r < a.N) op[r] = f2bf(y[r]);
                }
            }
        } else {  // SK_BIAS_F32: logits (+ arg-max partial of this 16-column tile)
            logits_epilogue<LSE>(a, y, m, mvalid, n, fq, blockIdx.x, gridDim.x);
        }
    }
}

// The single-wave vocabulary head of the scoring pass (gitcap_score behind gitcap_dbg_config(10, 0), or fewer than four tiles): the
// SK_BIAS_F32 path of skinny_full_kernel with the three partials and the target logit (logits_epilogue<true, true>) -- a kernel of
// its own, so that skinny_full_kernel stays the code it was.  Same operands, same MFMA chain, same bits.  The target of the lane's
// row is requested ahead of the activation fragments of its m-tile (vmcnt counts in order: the epilogue that needs it leaves the
// next m-tile's fragments in flight).
template <int K32, bool FP8>
__global__ __launch_bounds__(64) void skinny_full_score_kernel(SkinnyArgs a, HeadTargets tg) {
    const int lane = threadIdx.x;
    const int frow = lane & 15, fq = lane >> 4;
    const int n0 = blockIdx.x * 16;
    bf16x8 wf[K32];
    load_wfrags<K32, FP8>(a.W, a.Wpk, a.wscale, (size_t)(n0 + frow), a.K, fq * 8, wf);
    const int n = n0 + fq * 4;
    float bias[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[r] = (a.bias && n + r < a.N) ? a.bias[n + r] : 0.f;
    const int mtiles = (a.M + 15) >> 4;
    bf16x8 xnext[K32];
    int64_t tnext;
    auto load_x = [&](int mt) {
        const int m = min(mt * 16 + frow, a.M - 1);
        tnext = head_target(tg, m);
        const bf16_t* xp = a.X + (size_t)m * a.ldx + fq * 8;
#pragma unroll
        for (int k = 0; k < K32; ++k) xnext[k] = *(const bf16x8*)(xp + k * 32);
    };
    load_x(0);
    for (int mt = 0; mt < mtiles; ++mt) {
        const int m = mt * 16 + frow;
        bf16x8 xcur[K32];
#pragma unroll
        for (int k = 0; k < K32; ++k) xcur[k] = xnext[k];
        const int64_t tcol = tnext;
        if (mt + 1 < mtiles) load_x(mt + 1);
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < K32; ++k) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[k], xcur[k], acc, 0, 0, 0);
        float y[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] = acc[r] + bias[r];
        logits_epilogue<true, true>(a, y, min(m, a.M - 1), m < a.M, n, fq, blockIdx.x, gridDim.x, tcol, tg.logit);
    }
}

// The single-wave vocabulary head under a ban mask (gitcap_dbg_config(10, 0), fewer than four tiles, K = 1024): the SK_BIAS_F32 path
// of skinny_full_kernel with the banned columns of the lane's row written -inf ahead of the epilogue (skinny_head_body's BAN
// form: same rule, same bits) -- a kernel of its own, as skinny_full_score_kernel.  The row's mask word of this tile is requested
// ahead of the activation fragments of its m-tile.
template <int K32, bool FP8, bool LSE>
__global__ __launch_bounds__(64) void skinny_full_ban_kernel(SkinnyArgs a, HeadBan bn) {
    const int lane = threadIdx.x;
    const int frow = lane & 15, fq = lane >> 4;
    const int n0 = blockIdx.x * 16;
    bf16x8 wf[K32];
    load_wfrags<K32, FP8>(a.W, a.Wpk, a.wscale, (size_t)(n0 + frow), a.K, fq * 8, wf);
    const int n = n0 + fq * 4;
    float bias[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[r] = (a.bias && n + r < a.N) ? a.bias[n + r] : 0.f;
    const int mtiles = (a.M + 15) >> 4;
    bf16x8 xnext[K32];
    unsigned bnext;
    auto load_x = [&](int mt) {
        const int m = min(mt * 16 + frow, a.M - 1);
        bnext = bn.mask[(size_t)m * bn.ld + blockIdx.x];
        const bf16_t* xp = a.X + (size_t)m * a.ldx + fq * 8;
#pragma unroll
        for (int k = 0; k < K32; ++k) xnext[k] = *(const bf16x8*)(xp + k * 32);
    };
    load_x(0);
    for (int mt = 0; mt < mtiles; ++mt) {
        const int m = mt * 16 + frow;
        bf16x8 xcur[K32];
#pragma unroll
        for (int k = 0; k < K32; ++k) xcur[k] = xnext[k];
        const unsigned bcur = bnext;
        if (mt + 1 < mtiles) load_x(mt + 1);
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < K32; ++k) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[k], xcur[k], acc, 0, 0, 0);
        float y[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] = ((bcur >> (fq * 4 + r)) & 1u) ? -INFINITY : acc[r] + bias[r];
        logits_epilogue<LSE>(a, y, min(m, a.M - 1), m < a.M, n, fq, blockIdx.x, gridDim.x);
    }
}

// ---- vocabulary head with shared activation rows ------------------------------------------------------------------------
// skinny_full with SK_BIAS_F32 runs one single-wave workgroup per 16-column tile and every one of them fetches the same
// 16 x K activation tile -- at K = 768 as many bytes as the weight tile it owns, 1908 times over for the 30522-word
// vocabulary (through L2, but through the CU's one vector-memory port all the same).  Here four waves = four neighbouring
// tiles form a workgroup that fetches the activation m-tile ONCE, into LDS (row pitch + 16 B: the 16 lanes of a
// ds_read_b128 group fall into 16 different 16-byte slots), requested ahead of the weight fragments so that the LDS copy
// waits for it alone (vmcnt counts in order) while the weights stay in flight; m-tile mt + 1 is in flight under m-tile mt
// (two LDS images).  Every output element is the same MFMA chain over the same operands as in skinny_full: same bits.
// BAN (constrained decoding; kernels.h: HeadBan): the lane that holds columns n .. n + 3 of row m reads the row's mask word of its
// tile -- one uint16 = the tile's 16 columns, its bits fq * 4 .. fq * 4 + 3 -- and writes -inf into the banned y[r] before the
// epilogue forms a.out, the arg-max partial and the sum partial: a banned maximum leaves the runner-up, a wholly banned tile the
// empty partial (-inf, 0x7fffffff, sum 0).  The edit sits where the reference edits its logits (model.py:522-531, ahead of the
// log_softmax at :557), so the probabilities renormalise over the allowed columns -- unlike HF's beam search, which masks after
// normalising.  The word is requested like TGT's target, ahead of the activation rows of its m-tile: the LDS copy's counted wait
// covers it.  Kernels of their own, picked by the launcher where a mask is attached.
template <int K32, bool FP8, bool LSE, bool TGT = false, bool BAN = false>
__device__ __forceinline__ void skinny_head_body(const SkinnyArgs a, const int ntiles, const HeadTargets tg = HeadTargets{},
                                                 const HeadBan bn = HeadBan{}) {
    constexpr int PITCH = K32 * 64 + 16, CPR = K32 * 4, NC = (16 * CPR + 255) / 256;     // 16 x CPR 16-byte pieces over 256 threads
    __shared__ __attribute__((aligned(16))) char xs[2][16 * PITCH];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int frow = lane & 15, fq = lane >> 4;
    const int tile_raw = blockIdx.x * 4 + wave;
    const bool active = tile_raw < ntiles;                       // the last workgroup may hold fewer than four tiles: such a
    const int tile = active ? tile_raw : ntiles - 1;             // wave repeats the last tile and stores nothing
    const int n0 = tile * 16;
    const int mtiles = (a.M + 15) >> 4;
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    u32x4 st[NC];
    auto gload = [&](int mt) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int c0 = (int)threadIdx.x + 256 * i, c = c0 < 16 * CPR ? c0 : 0;      // (K = 576: 4.5 pieces per thread)
            const int row = c / CPR, col = c - row * CPR;
            int m = mt * 16 + row;
            m = m < a.M ? m : a.M - 1;                           // clamp: padded rows are discarded
            st[i] = *(const u32x4*)(a.X + (size_t)m * a.ldx + col * 8);
        }
    };
    auto lstore = [&](int buf) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int c = (int)threadIdx.x + 256 * i, row = c / CPR, col = c - row * CPR;
            if (c < 16 * CPR) *(u32x4*)(&xs[buf][row * PITCH + col * 16]) = st[i];
        }
    };
    // TGT: the target of the lane's row of m-tile mt, requested ahead of the activation rows of that m-tile: the LDS copy's wait
    // covers it and leaves the same requests in flight as before
    int64_t tnext = -1;
    if (TGT) tnext = head_target(tg, min(frow, a.M - 1));
    unsigned bnext = 0u;
    if (BAN) bnext = bn.mask[(size_t)min(frow, a.M - 1) * bn.ld + tile];
    gload(0);
    bf16x8 wf[K32];
    load_wfrags<K32, FP8>(a.W, a.Wpk, a.wscale, (size_t)(n0 + frow), a.K, fq * 8, wf);
    const int n = n0 + fq * 4;
    float bias[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[r] = (a.bias && n + r < a.N) ? a.bias[n + r] : 0.f;
    lstore(0);
    __syncthreads();
    for (int mt = 0; mt < mtiles; ++mt) {
        const int64_t tcol = tnext;
        const unsigned bcur = bnext;
        if (mt + 1 < mtiles) {
            if (TGT) tnext = head_target(tg, min((mt + 1) * 16 + frow, a.M - 1));
            if (BAN) bnext = bn.mask[(size_t)min((mt + 1) * 16 + frow, a.M - 1) * bn.ld + tile];
            gload(mt + 1);
        }
        const char* xb = &xs[mt & 1][frow * PITCH + fq * 16];
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < K32; ++k) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[k], *(const bf16x8*)(xb + k * 64), acc, 0, 0, 0);
        const int m = mt * 16 + frow;
        const bool mvalid = m < a.M && active;
        float y[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] = acc[r] + bias[r];
        if (BAN) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if ((bcur >> (fq * 4 + r)) & 1u) y[r] = -INFINITY;
        }
        logits_epilogue<LSE, TGT>(a, y, m < a.M ? m : a.M - 1, mvalid, n, fq, tile, ntiles, tcol, tg.logit);
        if (mt + 1 < mtiles) lstore((mt + 1) & 1);              // the image m-tile mt - 1 was read from: every wave is past the
        __syncthreads();                                         // barrier that closed that iteration
    }
}

template <int K32, bool FP8>
__global__ __launch_bounds__(256) void skinny_head_kernel(SkinnyArgs a, const int ntiles) { skinny_head_body<K32, FP8, false>(a, ntiles); }
// the same kernel with the third partial of the token log-probabilities (logits_epilogue<true>)
template <int K32, bool FP8>
__global__ __launch_bounds__(256) void skinny_head_lse_kernel(SkinnyArgs a, const int ntiles) { skinny_head_body<K32, FP8, true>(a, ntiles); }
// the scoring pass: the three partials + the logit of each row's given next token (logits_epilogue<true, true>)
template <int K32, bool FP8>
__global__ __launch_bounds__(256) void skinny_head_score_kernel(SkinnyArgs a, const int ntiles, HeadTargets tg) {
    skinny_head_body<K32, FP8, true, true>(a, ntiles, tg);
}
// constrained decoding: the plain and the LSE head with the ban mask applied (skinny_head_body<.., BAN = true>)
template <int K32, bool FP8, bool LSE>
__global__ __launch_bounds__(256) void skinny_head_ban_kernel(SkinnyArgs a, const int ntiles, HeadBan bn) {
    skinny_head_body<K32, FP8, LSE, false, true>(a, ntiles, HeadTargets{}, bn);
}

// ---- two vocabulary heads over the same tile: teacher-student divergence (gitcap_distill) -----------------------------------
// KL(teacher || student) of a row needs sum_v p_t(v) (t_v - s_v): both models' logits of the same column at the same time.  The
// workgroup of skinny_head_body -- four waves = four neighbouring 16-column tiles -- here keeps the fragments of BOTH head weights
// of its tile (KT + KS bf16x8 registers per lane: 42 at 768 + 576, 50 at 1024 + 576), stages both activation m-tiles through LDS
// (pitch rule as above, two images) and runs two MFMA chains per m-tile, teacher then student, each over the operands and in the
// order of the single-head kernels: t and s are bit for bit the logits those kernels produce.  No logit is stored.  Per (row, tile)
// it leaves, with t = (acc + bias) * inv_temp and s likewise, over the columns < N:
//     t_max / t_idx / t_sum, s_max / s_idx / s_sum   logits_epilogue<true>'s three partials of each model (same code order: the
//                                                    lane's columns ascending, then the 16 / 32 xor butterfly; inv_temp == 1: same bits)
//     cross = sum exp(t - t_max) ((t - t_max) - (s - s_max))   over the columns with t > -inf; the exp is the very value summed
//                                                    into t_sum.  +inf outright where such a column has s = -inf (never 0 * inf,
//                                                    never -inf - -inf); 0 for a tile whose t_max is -inf.
// launch_distill_final (select.hip) re-centres with the tile maxima and merges in a fixed order.
// LDS: 2 x 16 x ((KT + KS) * 64 + 32) bytes = 87 040 at 768 + 576, 103 424 at 1024 + 576, 13 312 at 128 + 64: one workgroup per CU
// at the model sizes (160 KiB per CU), i.e. one wave per SIMD with the whole 512-register file to itself -- the fragments of both
// weights (168 / 200 registers) stay resident across the m-tiles without scratch.  The launch streams both weights once (82 MB
// at the GIT vocabulary) and is bound by that stream like the single heads.
template <int K32> struct XTile {
    static constexpr int PITCH = K32 * 64 + 16, CPR = K32 * 4, NC = (16 * CPR + 255) / 256, BYTES = 16 * PITCH;
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    u32x4 st[NC];
    __device__ __forceinline__ void gload(const bf16_t* X, const int ldx, const int M, const int mt) {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int c0 = (int)threadIdx.x + 256 * i, c = c0 < 16 * CPR ? c0 : 0;
            const int row = c / CPR, col = c - row * CPR;
            int m = mt * 16 + row;
            m = m < M ? m : M - 1;                               // clamp: padded rows are discarded
            st[i] = *(const u32x4*)(X + (size_t)m * ldx + col * 8);
        }
    }
    __device__ __forceinline__ void lstore(char* img) const {
#pragma unroll
        for (int i = 0; i < NC; ++i) {
            const int c = (int)threadIdx.x + 256 * i, row = c / CPR, col = c - row * CPR;
            if (c < 16 * CPR) *(u32x4*)(&img[row * PITCH + col * 16]) = st[i];
        }
    }
};

// logits_epilogue<true>'s three partials of one model's 16 x 16 tile, in its order; e[r] = the exp terms summed into se (0 for
// a column that is not counted)
__device__ __forceinline__ void dual_tile_stats(const float (&y)[4], const int n, const int N, float& best, int& bi, float& se, float (&e)[4]) {
    best = -INFINITY;
    bi = 0x7fffffff;
#pragma unroll
    for (int r = 0; r < 4; ++r)
        if (n + r < N && (y[r] > best)) { best = y[r]; bi = n + r; }
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) {
        const float v2 = __shfl_xor(best, off);
        const int i2 = __shfl_xor(bi, off);
        if (v2 > best || (v2 == best && i2 < bi)) { best = v2; bi = i2; }
    }
    se = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) e[r] = 0.f;
    if (best != -INFINITY) {
#pragma unroll
        for (int r = 0; r < 4; ++r)
            if (n + r < N) { e[r] = __expf(y[r] - best); se += e[r]; }
    }
#pragma unroll
    for (int off = 16; off < 64; off <<= 1) se += __shfl_xor(se, off);
}

template <int KT, int KS, bool FP8>
__global__ __launch_bounds__(256) void skinny_head_dual_kernel(const DualHeadArgs a, const int ntiles) {
    typedef XTile<KT> TT;
    typedef XTile<KS> TS;
    constexpr int IMG = TT::BYTES + TS::BYTES;
    __shared__ __attribute__((aligned(16))) char xs[2][IMG];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int frow = lane & 15, fq = lane >> 4;
    const int tile_raw = blockIdx.x * 4 + wave;
    const bool active = tile_raw < ntiles;                       // (a wave past the last tile repeats it and stores nothing)
    const int tile = active ? tile_raw : ntiles - 1;
    const int n0 = tile * 16, N = a.wt.V;
    const int mtiles = (a.M + 15) >> 4;
    const bool tgt = a.tg.ids != nullptr;
    TT xt;
    TS xst;
    int64_t tnext = -1;
    if (tgt) tnext = head_target(a.tg, min(frow, a.M - 1));
    xt.gload(a.Xt, a.ldxt, a.M, 0);
    xst.gload(a.Xs, a.ldxs, a.M, 0);
    bf16x8 wt[KT], ws[KS];
    load_wfrags<KT, FP8>(a.wt.W, a.wt.Wpk, a.wt.wscale, (size_t)(n0 + frow), KT * 32, fq * 8, wt);
    load_wfrags<KS, false>(a.ws.W, a.ws.Wpk, nullptr, (size_t)(n0 + frow), KS * 32, fq * 8, ws);
    const int n = n0 + fq * 4;
    float bt[4], bs[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        bt[r] = (a.wt.bias && n + r < N) ? a.wt.bias[n + r] : 0.f;
        bs[r] = (a.ws.bias && n + r < N) ? a.ws.bias[n + r] : 0.f;
    }
    xt.lstore(&xs[0][0]);
    xst.lstore(&xs[0][TT::BYTES]);
    __syncthreads();
    for (int mt = 0; mt < mtiles; ++mt) {
        const int64_t tcol = tnext;
        if (mt + 1 < mtiles) {
            if (tgt) tnext = head_target(a.tg, min((mt + 1) * 16 + frow, a.M - 1));
            xt.gload(a.Xt, a.ldxt, a.M, mt + 1);
            xst.gload(a.Xs, a.ldxs, a.M, mt + 1);
        }
        const char* xbt = &xs[mt & 1][frow * TT::PITCH + fq * 16];
        const char* xbs = &xs[mt & 1][TT::BYTES + frow * TS::PITCH + fq * 16];
        f32x4 acct = f32x4{0.f, 0.f, 0.f, 0.f}, accs = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KT; ++k) acct = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wt[k], *(const bf16x8*)(xbt + k * 64), acct, 0, 0, 0);
#pragma unroll
        for (int k = 0; k < KS; ++k) accs = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ws[k], *(const bf16x8*)(xbs + k * 64), accs, 0, 0, 0);
        const int mraw = mt * 16 + frow, m = mraw < a.M ? mraw : a.M - 1;
        const bool mvalid = mraw < a.M && active;
        float t[4], sv[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            t[r] = (acct[r] + bt[r]) * a.inv_temp;
            sv[r] = (accs[r] + bs[r]) * a.inv_temp;
        }
        if (mvalid && tcol >= n && tcol < n + 4 && tcol < N) {
#pragma unroll
            for (int r = 0; r < 4; ++r)                         // (one store each, as logits_epilogue<.., true>)
                if (tcol == n + r) { a.tg.logit[m] = t[r]; a.s_logit[m] = sv[r]; }
        }
        float tb, sb, tse, sse, te[4], se4[4];
        int ti, si;
        dual_tile_stats(t, n, N, tb, ti, tse, te);
        dual_tile_stats(sv, n, N, sb, si, sse, se4);
        float cr = 0.f;
        if (tb != -INFINITY) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (n + r < N && t[r] != -INFINITY) cr += sv[r] == -INFINITY ? INFINITY : te[r] * ((t[r] - tb) - (sv[r] - sb));
        }
#pragma unroll
        for (int off = 16; off < 64; off <<= 1) cr += __shfl_xor(cr, off);
        if (fq == 0 && mvalid) {
            const size_t o = (size_t)m * ntiles + tile;
            a.t_max[o] = tb; a.t_idx[o] = ti; a.t_sum[o] = tse;
            a.s_max[o] = sb; a.s_idx[o] = si; a.s_sum[o] = sse;
            a.cross[o] = cr;
        }
        if (mt + 1 < mtiles) {                                   // the image m-tile mt - 1 was read from (skinny_head_body)
            xt.lstore(&xs[(mt + 1) & 1][0]);
            xst.lstore(&xs[(mt + 1) & 1][TT::BYTES]);
        }
        __syncthreads();
    }
}

template <int KT, int KS>
hipError_t launch_dual(const DualHeadArgs& a, const int ntiles, hipStream_t s) {
    if (a.wt.wscale) hipLaunchKernelGGL((skinny_head_dual_kernel<KT, KS, true>), dim3((ntiles + 3) / 4), dim3(256), 0, s, a, ntiles);
    else hipLaunchKernelGGL((skinny_head_dual_kernel<KT, KS, false>), dim3((ntiles + 3) / 4), dim3(256), 0, s, a, ntiles);
    return hipGetLastError();
}

// ---- top-k alternatives of a head row (kernels.h: HeadTopkArgs) -----------------------------------------------------------------
// One 256-thread workgroup per output row, behind the LSE head that left the row's three partials.
//   1. the row's bf16 activations and (up to TOPK_PART tiles; beyond that they are read from L2 every round) its arg-max partials go
//      to LDS; k rounds pick the k best tiles by (val descending, idx ascending): round r takes the best tile strictly behind round
//      r - 1's pick -- the pairs of non-empty tiles are all different -- and the rounds end early where no tile is left.  Empty tiles
//      (idx 0x7fffffff) are never picked.
//   2. lp_partials: the row's -log(z) against M = round 0's val, the winner's logit.
//   3. the four waves walk the picked tiles: load_wfrags, then skinny_head_body's chain -- the weight fragments in the A operand,
//      the row in all 16 columns of the B operand (an MFMA output element depends on its own A row and B column alone: the head's
//      bits, whatever the head's m-tile held beside this row) -- bias, the ban word of (row, tile), columns >= V as -inf; the lanes
//      of B column 0 leave the 16 logits in LDS.
//   4. every candidate above -inf counts the candidates ahead of it under (logit descending, column ascending); a rank below k
//      writes its column and (logit - M) + (-log z).  Ranks nobody takes keep -1 / -inf.
struct HeadTopkK {
    const bf16_t* X; int ldx;
    const void *W, *Wpk; const float *wscale, *bias; int V;
    const float* val; const int* idx; const float* sum; int ntiles;
    const uint16_t* mask; int ld_mask;
    int T, row_stride, row_off, k;
    int64_t* top_ids; float* top_lp; int ld;
};
constexpr int TOPK_PART = 2048;
template <int K32, bool FP8>
__global__ __launch_bounds__(256) void head_topk_kernel(const HeadTopkK a) {
    __shared__ __attribute__((aligned(16))) bf16_t xrow[K32 * 32];
    __shared__ float pv[TOPK_PART];
    __shared__ int pi[TOPK_PART];
    __shared__ float sv[2][4], ss[4], lpw_s, olp[HEAD_TOPK_MAX];
    __shared__ int si[2][4], sel_col[HEAD_TOPK_MAX], oid[HEAD_TOPK_MAX];
    __shared__ __attribute__((aligned(16))) float cand[HEAD_TOPK_MAX * 16];
    typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int frow = lane & 15, fq = lane >> 4;
    const int orow = blockIdx.x / a.T, opos = blockIdx.x - orow * a.T;
    const size_t m = (size_t)orow * a.row_stride + a.row_off + opos;
    const size_t base = m * a.ntiles;
    const int ntiles = a.ntiles, k = a.k;
    if (tid < K32 * 4) *(u32x4*)(&xrow[tid * 8]) = *(const u32x4*)(a.X + m * a.ldx + tid * 8);
    const bool part_lds = ntiles <= TOPK_PART;
    if (part_lds)
        for (int i = tid; i < ntiles; i += 256) { pv[i] = a.val[base + i]; pi[i] = a.idx[base + i]; }
    if (tid < HEAD_TOPK_MAX) { oid[tid] = -1; olp[tid] = -INFINITY; }
    __syncthreads();
    // 1. the k best tiles
    float pval = INFINITY, rowmax = -INFINITY;
    int pidx = -1, nsel = 0;
    for (int r = 0; r < k; ++r) {
        float best = -INFINITY;
        int bi = 0x7fffffff;
        for (int i = tid; i < ntiles; i += 256) {
            const float v = part_lds ? pv[i] : a.val[base + i];
            const int c = part_lds ? pi[i] : a.idx[base + i];
            const bool behind = v < pval || (v == pval && c > pidx);
            if (c != 0x7fffffff && behind && (v > best || (v == best && c < bi))) { best = v; bi = c; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float v2 = __shfl_xor(best, o);
            const int i2 = __shfl_xor(bi, o);
            if (v2 > best || (v2 == best && i2 < bi)) { best = v2; bi = i2; }
        }
        if (lane == 0) { sv[r & 1][wave] = best; si[r & 1][wave] = bi; }
        __syncthreads();                                         // (round r + 2 reuses this pair behind round r + 1's barrier)
        best = sv[r & 1][0];
        bi = si[r & 1][0];
#pragma unroll
        for (int w = 1; w < 4; ++w)
            if (sv[r & 1][w] > best || (sv[r & 1][w] == best && si[r & 1][w] < bi)) { best = sv[r & 1][w]; bi = si[r & 1][w]; }
        if (bi == 0x7fffffff) break;                             // (uniform) no tile left
        pval = best;
        pidx = bi;
        if (r == 0) rowmax = best;
        if (tid == 0) sel_col[r] = min(max(bi, 0) >> 4, ntiles - 1) << 4;     // (a partial is a column < V: the clamp never acts)
        nsel = r + 1;
    }
    // 2. -log z of the row (one barrier inside: sel_col and xrow are visible behind it)
    const float lpw0 = lp_partials(a.val, a.sum, base, ntiles, rowmax, ss);
    if (tid == 0) lpw_s = lpw0;
    // 3. the picked tiles' logits
    for (int t = wave; t < nsel; t += 4) {
        const int n0 = sel_col[t];
        bf16x8 wf[K32];
        load_wfrags<K32, FP8>(a.W, a.Wpk, a.wscale, (size_t)(n0 + frow), K32 * 32, fq * 8, wf);
        const unsigned bw = a.mask ? a.mask[m * a.ld_mask + (n0 >> 4)] : 0u;
        const int n = n0 + fq * 4;
        float bias[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) bias[r] = (a.bias && n + r < a.V) ? a.bias[n + r] : 0.f;
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < K32; ++kk)
            acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[kk], *(const bf16x8*)(&xrow[fq * 8 + kk * 32]), acc, 0, 0, 0);
        f32x4 y;
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] = (n + r >= a.V || ((bw >> (fq * 4 + r)) & 1u)) ? -INFINITY : acc[r] + bias[r];
        if (frow == 0) *(f32x4*)(&cand[t * 16 + fq * 4]) = y;
    }
    __syncthreads();
    // 4. rank the candidates
    const int ncand = nsel * 16;
    const float lpw = lpw_s;
    for (int q = tid; q < ncand; q += 256) {
        const float v = cand[q];
        const int c = sel_col[q >> 4] + (q & 15);
        if (!(v > -INFINITY)) continue;
        int rank = 0;
        for (int p = 0; p < ncand; p += 4) {
            const f32x4 o = *(const f32x4*)(&cand[p]);
            const int c0 = sel_col[p >> 4] + (p & 15);
#pragma unroll
            for (int u = 0; u < 4; ++u) rank += (o[u] > v || (o[u] == v && c0 + u < c)) ? 1 : 0;
        }
        if (rank < k) { oid[rank] = c; olp[rank] = (v - rowmax) + lpw; }
    }
    __syncthreads();
    if (tid < k) {
        const size_t o = ((size_t)orow * a.ld + opos) * k + tid;
        a.top_ids[o] = oid[tid];
        a.top_lp[o] = olp[tid];
    }
}

template <int K32, bool FP8>
hipError_t launch_topk(const HeadTopkK& kk, int nrows, hipStream_t s) {
    hipLaunchKernelGGL((head_topk_kernel<K32, FP8>), dim3(nrows), dim3(256), 0, s, kk);
    return hipGetLastError();
}

// ---- one/two-row prologue over many slabs: three waves share the reduce ---------------------------------------------------
// The fused FFN launch (ffn_txt.hip) leaves dec_ffn / 64 = 48 slabs; the single wave of skinny_full<LNR> walks them in three
// dependent round trips (two 8-slab groups each) before it can normalise its row -- in every one of the 144 workgroups, 150
// times per single-clip caption.  Here a workgroup is three waves = three neighbouring 16-column tiles: wave w sums groups
// 2w and 2w + 1 of the row (one round trip, side by side), waves 1 and 2 hand their group sums over through LDS, wave 0 adds
// them in the canonical order (rowln.h: 0 + t0 + t1 + ... ascending; the same adds as row_load_reduce and ln_reduce_kernel),
// adds bias + residual, normalises and leaves the bf16 row in LDS; then every wave runs its own tile's MFMA chain.  Same bits.
template <int K32, int EPI>
__global__ __launch_bounds__(192) void skinny_rows3_kernel(SkinnyArgs a) {
    constexpr int NV = (K32 * 32 + 255) / 256;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int frow = lane & 15, fq = lane >> 4;
    const int ntiles = (a.N + 15) / 16;
    const int tile_raw = blockIdx.x * 3 + wave;
    const bool active = tile_raw < ntiles;                       // (a wave past the last tile repeats it and stores nothing)
    const int n0 = (active ? tile_raw : ntiles - 1) * 16;
    bf16x8 wf[K32];
    load_wfrags<K32, false>(a.W, a.Wpk, a.wscale, (size_t)(n0 + frow), a.K, fq * 8, wf);
    __shared__ __attribute__((aligned(16))) bf16_t xrow[2][K32 * 32];
    __shared__ __attribute__((aligned(16))) float part[2][2][NV * 256];        // group sums of waves 1, 2
    const SkinnyArgs::RowPrologue& p = a.ln;
    const int ngroups = (p.nslab + 7) >> 3;
    for (int m = 0; m < a.M; ++m) {
        // what wave 0 needs after the merge: requested by every wave ahead of the slabs (a branch around loads is waited for where
        // it ends), in flight behind the trees
        f32x4 bv[NV], rv[NV], gv[NV], bev[NV];
        row_load_vec<NV>(bv, p.bias, a.K, lane);
        row_load_vec<NV>(rv, p.resid + (size_t)m * a.K, a.K, lane);
        row_load_vec<NV>(gv, p.g, a.K, lane);
        row_load_vec<NV>(bev, p.b, a.K, lane);
        f32x4 ta[NV], tb[NV];
        row_slab_tree<NV>(ta, p.slabs, p.nslab, wave * 16, a.M, a.K, m, lane);
        row_slab_tree<NV>(tb, p.slabs, p.nslab, wave * 16 + 8, a.M, a.K, m, lane);
        if (wave > 0) {
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                *(f32x4*)(&part[wave - 1][0][i * 256 + lane * 4]) = ta[i];
                *(f32x4*)(&part[wave - 1][1][i * 256 + lane * 4]) = tb[i];
            }
        }
        __syncthreads();
        if (wave == 0) {
            f32x4 v[NV];
#pragma unroll
            for (int i = 0; i < NV; ++i) { v[i] = f32x4{0.f, 0.f, 0.f, 0.f}; v[i] += ta[i]; }
            if (ngroups > 1) {
#pragma unroll
                for (int i = 0; i < NV; ++i) v[i] += tb[i];
            }
            for (int g = 2; g < ngroups; ++g)
#pragma unroll
                for (int i = 0; i < NV; ++i) v[i] += *(const f32x4*)(&part[(g >> 1) - 1][g & 1][i * 256 + lane * 4]);
            const float s = row_add_bias_resid_v<NV>(v, bv, rv, a.K, lane);
            row_layernorm_v<NV>(v, s, lane, a.K, p.eps, gv, bev);
            row_store<NV>(v, lane, a.K, blockIdx.x == 0 ? p.xf + (size_t)m * a.K : nullptr, (bf16_t*)nullptr);
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                const int c = i * 256 + lane * 4;
                if (c < K32 * 32) {
                    uint2 o;
                    o.x = pack_bf2(v[i][0], v[i][1]);
                    o.y = pack_bf2(v[i][2], v[i][3]);
                    *(uint2*)(&xrow[m][c]) = o;
                }
            }
        }
        __syncthreads();                                        // the row is in LDS; `part` may be overwritten
    }
    const int n = n0 + fq * 4;
    float bias[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) bias[r] = (a.bias && n + r < a.N) ? a.bias[n + r] : 0.f;
    int m = frow;
    const bool mvalid = m < a.M && active;
    m = m < a.M ? m : a.M - 1;
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int k = 0; k < K32; ++k) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[k], *(const bf16x8*)(&xrow[m][fq * 8 + k * 32]), acc, 0, 0, 0);
    float y[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) y[r] = acc[r] + bias[r];
    if (EPI == SK_BIAS_RELU_BF16) {
#pragma unroll
        for (int r = 0; r < 4; ++r) y[r] = fmaxf(y[r], 0.f);
    }
    if (mvalid) {
        const int orow = (m / a.T) * a.row_stride + a.row_off + (m % a.T);
        bf16_t* op = (bf16_t*)a.out + (size_t)orow * a.ldo + n;
        if (n + 3 < a.N) {
            uint2 v;
            v.x = pack_bf2(y[0], y[1]);
            v.y = pack_bf2(y[2], y[3]);
            *(uint2*)op = v;
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (n + r < a.N) op[r] = f2bf(y[r]);
        }
    }
}

// grid = (n_tiles, ksplit); slab[ks][m][n] fp32 partial sums (no bias)
template <int K32, bool FP8>
__global__ __launch_bounds__(64) void skinny_splitk_kernel(SkinnyArgs a) {
    const int lane = threadIdx.x;
    const int frow = lane & 15, fq = lane >> 4;
    const int n0 = blockIdx.x * 16, ks = blockIdx.y;
    const int kbeg = ks * K32 * 32;
    bf16x8 wf[K32];
    load_wfrags<K32, FP8>(a.W, a.Wpk, a.wscale, (size_t)(n0 + frow), a.K, kbeg + fq * 8, wf);
    const int n = n0 + fq * 4;
    float* slab = (float*)a.out + (size_t)ks * a.M * a.ldo;
    const int mtiles = (a.M + 15) >> 4;
    bf16x8 xnext[K32];                                          // m-tile mt + 1's fragments in flight under m-tile mt (skinny_full)
    auto load_x = [&](int mt) {
        int m = mt * 16 + frow;
        m = m < a.M ? m : a.M - 1;
        const bf16_t* xp = a.X + (size_t)m * a.ldx + kbeg + fq * 8;
#pragma unroll
        for (int k = 0; k < K32; ++k) xnext[k] = *(const bf16x8*)(xp + k * 32);
    };
    load_x(0);
    for (int mt = 0; mt < mtiles; ++mt) {
        int m = mt * 16 + frow;
        const bool mvalid = m < a.M;
        m = mvalid ? m : a.M - 1;
        bf16x8 xcur[K32];
#pragma unroll
        for (int k = 0; k < K32; ++k) xcur[k] = xnext[k];
        if (mt + 1 < mtiles) load_x(mt + 1);
        f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < K32; ++k) acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[k], xcur[k], acc, 0, 0, 0);
        if (mvalid) *(f32x4*)(slab + (size_t)m * a.ldo + n) = acc;
    }
}

template <int K32, bool FP8>
hipError_t launch_full(const SkinnyArgs& a, int epi, hipStream_t s, const HeadTargets* tg, const HeadBan* bn) {
    const int grid = (a.N + 15) / 16;
    if (a.ln.kind) return hipErrorInvalidValue;          // row prologue: launch_full_rows
    const bool lse = a.amax_sum != nullptr;              // the third partial of the token log-probabilities: the <.., true> kernels
    if (lse && (epi != SK_BIAS_F32 || !a.amax_val || !a.amax_idx)) return hipErrorInvalidValue;
    // target capture (the scoring pass): kernels of their own, in the two forms of the head
    if (tg && (!lse || !tg->ids || !tg->logit || tg->T <= 0 || tg->ld < tg->T || tg->shift < 0 || a.M % tg->T)) return hipErrorInvalidValue;
    // ban mask (constrained decoding): kernels of their own, in the two forms of the head, plain or with the third partial
    if (bn && (tg || epi != SK_BIAS_F32 || !bn->mask || bn->ld < grid || (bn->ld & 1) || ((uintptr_t)bn->mask & 3) || (!a.out && !a.amax_val)))
        return hipErrorInvalidValue;
    if constexpr (K32 * 64 * 32 + 512 <= 64 * 1024) {          // two LDS images of 16 rows (K <= 768)
        // the vocabulary head (many tiles over few rows): four tiles per workgroup share the activation rows through LDS
        if (epi == SK_BIAS_F32 && g_head_share && grid >= 4 && a.ldx % 8 == 0 && ((uintptr_t)a.X & 15) == 0) {
            if (bn && lse) hipLaunchKernelGGL((skinny_head_ban_kernel<K32, FP8, true>), dim3((grid + 3) / 4), dim3(256), 0, s, a, grid, *bn);
            else if (bn) hipLaunchKernelGGL((skinny_head_ban_kernel<K32, FP8, false>), dim3((grid + 3) / 4), dim3(256), 0, s, a, grid, *bn);
            else if (tg) hipLaunchKernelGGL((skinny_head_score_kernel<K32, FP8>), dim3((grid + 3) / 4), dim3(256), 0, s, a, grid, *tg);
            else if (lse) hipLaunchKernelGGL((skinny_head_lse_kernel<K32, FP8>), dim3((grid + 3) / 4), dim3(256), 0, s, a, grid);
            else hipLaunchKernelGGL((skinny_head_kernel<K32, FP8>), dim3((grid + 3) / 4), dim3(256), 0, s, a, grid);
            return hipGetLastError();
        }
    }
    switch (epi) {
        case SK_BIAS_BF16: hipLaunchKernelGGL((skinny_full_kernel<K32, SK_BIAS_BF16, FP8, false>), dim3(grid), dim3(64), 0, s, a); break;
        case SK_BIAS_GELU_BF16: hipLaunchKernelGGL((skinny_full_kernel<K32, SK_BIAS_GELU_BF16, FP8, false>), dim3(grid), dim3(64), 0, s, a); break;
        case SK_BIAS_RELU_BF16: hipLaunchKernelGGL((skinny_full_kernel<K32, SK_BIAS_RELU_BF16, FP8, false>), dim3(grid), dim3(64), 0, s, a); break;
        case SK_BIAS_F32:
            if (bn && lse) hipLaunchKernelGGL((skinny_full_ban_kernel<K32, FP8, true>), dim3(grid), dim3(64), 0, s, a, *bn);
            else if (bn) hipLaunchKernelGGL((skinny_full_ban_kernel<K32, FP8, false>), dim3(grid), dim3(64), 0, s, a, *bn);
            else if (tg) hipLaunchKernelGGL((skinny_full_score_kernel<K32, FP8>), dim3(grid), dim3(64), 0, s, a, *tg);
            else if (lse) hipLaunchKernelGGL((skinny_full_kernel<K32, SK_BIAS_F32, FP8, false, true>), dim3(grid), dim3(64), 0, s, a);
            else hipLaunchKernelGGL((skinny_full_kernel<K32, SK_BIAS_F32, FP8, false, false>), dim3(grid), dim3(64), 0, s, a);
            break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// with the row prologue: a bf16-output projection of one or two text rows (GIT q|k|v; the student's q|k|v, cross q, FC1)
template <int K32>
hipError_t launch_full_rows(const SkinnyArgs& a, int epi, hipStream_t s) {
    const SkinnyArgs::RowPrologue& p = a.ln;
    if (!skinny_row_prologue_ok(a.M, a.K, a.wscale != nullptr) || !p.g || !p.b || !p.xf ||
        (p.kind == 1 && (!p.slabs || p.nslab <= 0 || !p.bias || !p.resid || p.resid == p.xf)) ||
        (p.kind == 2 && (!p.ids || p.T <= 0 || !p.word || !p.pos)) || (p.kind != 1 && p.kind != 2))
        return hipErrorInvalidValue;
    const dim3 grid((a.N + 15) / 16);
    // many slabs (the fused FFN's 48): three waves per workgroup share the reduce (skinny_rows3_kernel)
    if (g_rows3 && p.kind == 1 && p.nslab > 16 && p.nslab <= 48) {
        const dim3 grid3((grid.x + 2) / 3);
        if (epi == SK_BIAS_BF16) hipLaunchKernelGGL((skinny_rows3_kernel<K32, SK_BIAS_BF16>), grid3, dim3(192), 0, s, a);
        else if (epi == SK_BIAS_RELU_BF16) hipLaunchKernelGGL((skinny_rows3_kernel<K32, SK_BIAS_RELU_BF16>), grid3, dim3(192), 0, s, a);
        else return hipErrorInvalidValue;
        return hipGetLastError();
    }
    if (epi == SK_BIAS_BF16) hipLaunchKernelGGL((skinny_full_kernel<K32, SK_BIAS_BF16, false, true>), grid, dim3(64), 0, s, a);
    else if (epi == SK_BIAS_RELU_BF16) hipLaunchKernelGGL((skinny_full_kernel<K32, SK_BIAS_RELU_BF16, false, true>), grid, dim3(64), 0, s, a);
    else return hipErrorInvalidValue;
    return hipGetLastError();
}

}  // namespace

bool skinny_full_ok(int K) {
    const int k32 = K / 32;
    return K % 32 == 0 && (k32 == 2 || k32 == 4 || k32 == 8 || k32 == 18 || k32 == 24 || k32 == 32);
}

bool skinny_row_prologue_ok(int M, int K, bool fp8) { return M >= 1 && M <= 2 && (K == 64 || K == 128 || K == 576 || K == 768) && !fp8; }

hipError_t launch_skinny(const SkinnyArgs& a, int epi, hipStream_t s, const HeadTargets* tg, const HeadBan* bn) {
    if (a.K % 32 || a.M <= 0 || a.T <= 0) return hipErrorInvalidValue;
    if ((tg || bn) && (a.ln.kind || epi != SK_BIAS_F32)) return hipErrorInvalidValue;
    if (a.ln.kind)
        return a.K == 64 ? launch_full_rows<2>(a, epi, s) : a.K == 128 ? launch_full_rows<4>(a, epi, s)
             : a.K == 576 ? launch_full_rows<18>(a, epi, s) : launch_full_rows<24>(a, epi, s);
    if (a.wscale) {                                     // e4m3 weights (GIT decoder widths only)
        switch (a.K / 32) {
            case 4: return launch_full<4, true>(a, epi, s, tg, bn);
            case 24: return launch_full<24, true>(a, epi, s, tg, bn);
        }
        return hipErrorInvalidValue;
    }
    switch (a.K / 32) {
        case 2: return launch_full<2, false>(a, epi, s, tg, bn);      // K = 64  (tiny student test config)
        case 4: return launch_full<4, false>(a, epi, s, tg, bn);      // K = 128 (tiny test config)
        case 8: return launch_full<8, false>(a, epi, s, tg, bn);      // K = 256
        case 18: return launch_full<18, false>(a, epi, s, tg, bn);    // K = 576 (student decoder)
        case 24: return launch_full<24, false>(a, epi, s, tg, bn);    // K = 768
        case 32: return launch_full<32, false>(a, epi, s, tg, bn);    // K = 1024
    }
    return hipErrorInvalidValue;
}

// K slabs: 8 (else 16) for the K >= 2048 matrices, else the largest of 4, 3, 2 that leaves a supported per-slab depth
// (768 -> 4 x 6, 3072 -> 8 x 12, 4096 -> 16 x 8, 1024 -> 4 x 8; student decoder: 576 -> 3 x 6)
int skinny_ksplit(int K) {
    auto ok = [&](int ks) { const int k32 = K / (ks * 32); return K % (ks * 32) == 0 && (k32 == 1 || k32 == 2 || k32 == 6 || k32 == 8 || k32 == 12); };
    if (K >= 2048) return ok(8) ? 8 : (ok(16) ? 16 : 0);
    for (int ks = 4; ks >= 1; --ks)
        if (ok(ks)) return ks;
    return 0;
}

hipError_t launch_skinny_splitk(const SkinnyArgs& a, hipStream_t s) {
    const int ks = a.ksplit > 0 ? a.ksplit : skinny_ksplit(a.K);
    if (!ks || a.M <= 0 || a.N % 16 || a.K % (ks * 32)) return hipErrorInvalidValue;
    dim3 grid(a.N / 16, ks);
    if (a.wscale) {
        switch (a.K / ks / 32) {
            case 1: hipLaunchKernelGGL((skinny_splitk_kernel<1, true>), grid, dim3(64), 0, s, a); break;
            case 2: hipLaunchKernelGGL((skinny_splitk_kernel<2, true>), grid, dim3(64), 0, s, a); break;
            case 12: hipLaunchKernelGGL((skinny_splitk_kernel<12, true>), grid, dim3(64), 0, s, a); break;
            default: return hipErrorInvalidValue;
        }
        return hipGetLastError();
    }
    switch (a.K / ks / 32) {
        case 1: hipLaunchKernelGGL((skinny_splitk_kernel<1, false>), grid, dim3(64), 0, s, a); break;
        case 2: hipLaunchKernelGGL((skinny_splitk_kernel<2, false>), grid, dim3(64), 0, s, a); break;
        case 6: hipLaunchKernelGGL((skinny_splitk_kernel<6, false>), grid, dim3(64), 0, s, a); break;
        case 8: hipLaunchKernelGGL((skinny_splitk_kernel<8, false>), grid, dim3(64), 0, s, a); break;
        case 12: hipLaunchKernelGGL((skinny_splitk_kernel<12, false>), grid, dim3(64), 0, s, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

bool head_topk_ok(int D, bool fp8) {
    const int k32 = D / 32;
    if (D % 32) return false;
    return fp8 ? (k32 == 4 || k32 == 24) : skinny_full_ok(D);
}

hipError_t launch_head_topk(const HeadTopkArgs& a, hipStream_t s) {
    const int V = a.hw.V, D = a.hw.D, ntiles = (V + 15) / 16;
    const bool fp8 = a.hw.wscale != nullptr;
    if (!a.X || !a.hw.W || !a.val || !a.idx || !a.sum || !a.top_ids || !a.top_lp || V <= 0 || !head_topk_ok(D, fp8) ||
        a.k < 1 || a.k > HEAD_TOPK_MAX || a.rows <= 0 || a.T <= 0 || a.ld < a.T || a.row_stride < 0 || a.row_off < 0 ||
        a.ldx < D || a.ldx % 8 || ((uintptr_t)a.X & 15) || ((uintptr_t)a.top_ids & 7) || ((uintptr_t)a.top_lp & 3))
        return hipErrorInvalidValue;
    if (a.bn && (!a.bn->mask || a.bn->ld < ntiles)) return hipErrorInvalidValue;
    if (a.run_head) {
        // the last head row an output row reads lies inside the launch
        if (a.M <= 0 || (int64_t)(a.rows - 1) * a.row_stride + a.row_off + a.T - 1 >= a.M) return hipErrorInvalidValue;
        SkinnyArgs ha{};
        ha.X = a.X; ha.ldx = a.ldx; ha.W = a.hw.W; ha.Wpk = a.hw.Wpk; ha.wscale = a.hw.wscale; ha.bias = a.hw.bias;
        ha.M = a.M; ha.N = V; ha.K = D; ha.ldo = V; ha.T = 1; ha.row_stride = 1;
        ha.amax_val = a.val; ha.amax_idx = a.idx; ha.amax_sum = a.sum;
        const hipError_t e = launch_skinny(ha, SK_BIAS_F32, s, nullptr, a.bn);
        if (e != hipSuccess) return e;
    }
    const HeadTopkK kk{a.X, a.ldx, a.hw.W, a.hw.Wpk, a.hw.wscale, a.hw.bias, V, a.val, a.idx, a.sum, ntiles,
                       a.bn ? a.bn->mask : nullptr, a.bn ? a.bn->ld : 0, a.T, a.row_stride, a.row_off, a.k, a.top_ids, a.top_lp, a.ld};
    const int nrows = a.rows * a.T;
    if (fp8) return D == 128 ? launch_topk<4, true>(kk, nrows, s) : launch_topk<24, true>(kk, nrows, s);
    switch (D / 32) {
        case 2: return launch_topk<2, false>(kk, nrows, s);
        case 4: return launch_topk<4, false>(kk, nrows, s);
        case 8: return launch_topk<8, false>(kk, nrows, s);
        case 18: return launch_topk<18, false>(kk, nrows, s);
        case 24: return launch_topk<24, false>(kk, nrows, s);
        default: return launch_topk<32, false>(kk, nrows, s);
    }
}

bool head_dual_ok(int Kt, int Ks) { return (Kt == 128 && Ks == 64) || ((Kt == 768 || Kt == 1024) && Ks == 576); }

hipError_t launch_head_dual(const DualHeadArgs& a, hipStream_t s) {
    const int N = a.wt.V;
    if (!a.Xt || !a.Xs || !a.wt.W || !a.ws.W || a.ws.wscale || a.M <= 0 || N <= 0 || a.ws.V != N || !head_dual_ok(a.wt.D, a.ws.D) ||
        a.ldxt < a.wt.D || a.ldxs < a.ws.D || a.ldxt % 8 || a.ldxs % 8 || ((uintptr_t)a.Xt & 15) || ((uintptr_t)a.Xs & 15) ||
        !(a.inv_temp > 0.f) || a.inv_temp == INFINITY || !a.t_max || !a.t_idx || !a.t_sum || !a.s_max || !a.s_idx || !a.s_sum || !a.cross)
        return hipErrorInvalidValue;
    if (a.tg.ids && (!a.tg.logit || !a.s_logit || a.tg.T <= 0 || a.tg.ld < a.tg.T || a.tg.shift < 0 || a.M % a.tg.T)) return hipErrorInvalidValue;
    const int ntiles = (N + 15) / 16;
    switch (a.wt.D) {
        case 128: return launch_dual<4, 2>(a, ntiles, s);
        case 768: return launch_dual<24, 18>(a, ntiles, s);
        default: return launch_dual<32, 18>(a, ntiles, s);
    }
}
