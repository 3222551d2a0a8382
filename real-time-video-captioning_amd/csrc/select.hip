// The text rows' kernels around the decoder stack: token selection for greedy decoding and what else is built on the vocabulary
// head's per-tile partials (skinny.hip) -- the final arg-max with its prompt and keep forms, draft staging and verification, caption
// scoring, the distillation merge, the greedy loop's small kernels -- and, behind the arg-max, the two other users of rowln.h's row
// code: the text embedding (what the arg-max does for the next step's row) and the split-K reduce.  The three share a translation
// unit, the arg-max first, on purpose: what the compiler makes of each depends on which of the others it sees, and any of them left
// alone in a file compiles to other code (profiles/r28_rowops_split_resources.txt).  Topic by topic: the kernels, then their launchers.
#include "kernels.h"
#include "rowln.h"
#include "lp_partials.h"
#include "prompt_sel.h"

// ---- final arg-max over the per-tile partials written by the vocabulary-head kernel ------------
// The arg-max of one row's partials at val / idx + base by a 256-thread workgroup: the largest value, the smallest index among
// equals, 0 for an all-NaN row.  In two parts, both called by argmax_final_kernel and draft_accept_kernel (the one statement of the
// tie rule): argmax_partials_waves, by every thread, leaves each wave's candidate in sv / si (four words of LDS each) behind a
// barrier and thread 0's own in best / bi; argmax_partials_pick, by thread 0 alone, returns the row's.
namespace {
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
}  // namespace
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

// ---- text embedding + LayerNorm: one wave per (row, position) (rowln.h) --------------------------
namespace {
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
}  // namespace
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

// ---- split-K reduce + bias + residual + LayerNorm (text rows) (rowln.h) ---------------------------------------------
// One workgroup per row, one wave per group of 8 slabs: every wave sums its group (row_slab_tree), wave 0 adds the group
// sums in ascending order, then bias + residual, and normalises the row.  With up to 8 slabs that is one wave, the kernel of
// rounds 1-3; the fused FC1 -> GELU -> FC2 launch of round 4 (ffn_txt.hip) leaves dec_ffn / 64 = 48 slabs, 147 KB per
// row: six waves fetch them side by side.  Same bits as row_load_reduce in one wave (the row prologue of skinny.hip).
namespace {
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
}  // namespace
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
namespace {
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
}  // namespace
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

// ---- draft verification of the teacher's greedy loop, accepted row by row (gitcap.hip: greedy_draft_loop) -------------------
// column 0 = CLS whatever the draft holds, columns 1..n the draft's tokens, an id outside [0, vocab) as -1: the embedding clamps it
// into its table, it equals no arg-max, so it can only be rejected
namespace {
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
}  // namespace
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

// ---- scoring of given captions (gitcap_score; kernels.h: launch_score_final) ---------------------------------------------------
namespace {
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
}  // namespace
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
namespace {
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
}  // namespace
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

namespace {
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
}  // namespace
hipError_t launch_finish_steps(const int32_t* sep_cnt, int rows, int max_len, int stop, int32_t* steps_out, hipStream_t s) {
    hipLaunchKernelGGL(finish_steps_kernel, dim3(1), dim3(1), 0, s, sep_cnt, rows, max_len, stop, steps_out);
    return hipGetLastError();
}

hipError_t launch_fill_i64(int64_t* p, int ld, int rows, int64_t v, hipStream_t s) {
    hipLaunchKernelGGL(fill_i64_kernel, dim3((rows + 63) / 64), dim3(64), 0, s, p, ld, rows, v);
    return hipGetLastError();
}

hipError_t launch_fill_prompt(int64_t* p, int ld, int rows, const PromptArgs& prompt, hipStream_t s) {
    if (!p || !prompt.ids || !prompt.lengths || rows < 1 || prompt.max_len < 1 || prompt.ld < prompt.max_len || ld < prompt.max_len)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(fill_prompt_kernel, dim3((rows * prompt.max_len + 63) / 64), dim3(64), 0, s, p, ld, rows, prompt.ids, prompt.ld,
                       prompt.lengths, prompt.max_len);
    return hipGetLastError();
}
