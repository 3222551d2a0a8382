// Student caption decoder (SURVEY.md par. 8 row f.2): the reference's StudentCandidateV1 decoder
// (src/models/model.py:50-187 -- nn.TransformerDecoder, post-LN, ReLU, causal + key-padding mask,
// cross-attention over one memory token per frame) with an exact KV cache, behind the C ABI declared in
// include/gitcap.h ("student decoder" section).  The TinyViT image encoder is in tinyvit.hip.
//
// Everything here is the decode-loop regime of the GIT text path: M = rows x T is a handful of rows, so
// the dense layers are the weight-streaming skinny GEMMs (skinny.hip), the LayerNorms are fused with the
// split-K reduction (ln_reduce_kernel), and the two attentions (<= 64 keys) are one wave per (row, head).
//
// Exact KV cache: the self-attention K/V of position j depend only on tokens <= j and on the PAD flags
// of tokens <= j, so the reference's full recompute per step (model.py:173-177) and the cached loop agree.
#include "../../include/gitcap.h"
#include "kernels.h"
#include "host_util.h"
#include "student_internal.h"
#include "prompt_sel.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <map>
#include <string>
#include <vector>

namespace {

// ---- kernels -------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void student_embed_kernel(const int64_t* __restrict__ ids, int ld_ids, int T, int t0,
                                                           const float* __restrict__ embed, const float* __restrict__ pe,
                                                           int D, int vocab, float sqrt_d, float* __restrict__ xf,
                                                           bf16_t* __restrict__ xb) {
    const int m = blockIdx.x, r = m / T, pos = t0 + m % T;
    long long id = ids[(size_t)r * ld_ids + pos];
    id = id < 0 ? 0 : (id >= vocab ? vocab - 1 : id);
    const float* e = embed + (size_t)id * D;
    const float* p = pe + (size_t)pos * D;
    for (int c = threadIdx.x * 4; c < D; c += 256) {
        const f32x4 a = *(const f32x4*)(e + c), b = *(const f32x4*)(p + c);
        f32x4 y;
#pragma unroll
        for (int i = 0; i < 4; ++i) y[i] = (a[i] + b[i]) / sqrt_d;      // model.py:142-144: (embed + pe) / sqrt(D)
        *(f32x4*)(xf + (size_t)m * D + c) = y;
        uint2 o;
        o.x = pack_bf2(y[0], y[1]);
        o.y = pack_bf2(y[2], y[3]);
        *(uint2*)(xb + (size_t)m * D + c) = o;
    }
}

// one wave per (query, head); lane i owns key i for the scores and output column(s) lane, lane + 64 for P.V
// VL (clips of different length, gitcap_student_attach_frame_counts): the keys of decoder row r are the key_len[r] (1..64) packed
// memory rows from key_off[r] on -- device tables read at run time, so a captured loop follows the counts of the memory set last --
// instead of rows r * keys_stride .. + nkeys - 1.  Nothing else differs: a row with key_len = n has the bits of the plain form at
// nkeys = n.
template <bool VL>
__global__ __launch_bounds__(64) void attn_small_kernel(SmallAttnArgs a, const int32_t* __restrict__ key_off, const int32_t* __restrict__ key_len) {
    __shared__ float qs[128];
    __shared__ float ps[64];
    const int lane = threadIdx.x, m = blockIdx.x, h = blockIdx.y;
    const int r = m / a.T, j = m % a.T;
    int nk;
    if constexpr (VL) nk = min(max(key_len[r], 0), 64);
    else nk = a.nkeys > 0 ? a.nkeys : a.t0 + j + 1;
    const bf16_t* q = a.q + (size_t)(r * a.q_row_stride + a.q_row_off + j) * a.ldq + h * a.hd;
    for (int d = lane; d < a.hd; d += 64) qs[d] = bf2f(q[d]);
    __syncthreads();
    float s = -INFINITY;
    if (lane < nk) {
        const bf16_t* k;
        if constexpr (VL) k = a.k + (size_t)(key_off[r] + lane) * a.ldkv + h * a.hd;
        else k = a.k + (size_t)(r * a.keys_stride + lane) * a.ldkv + h * a.hd;
        float acc = 0.f;
        for (int c = 0; c < a.hd; c += 8) {
            const bf16x8 kk = *(const bf16x8*)(k + c);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc += qs[c + e] * bf2f((bf16_t)kk[e]);
        }
        const bool masked = a.ids && a.ids[(size_t)r * a.ld_ids + lane] == a.pad_id;
        s = masked ? -INFINITY : acc * rsqrtf((float)a.hd);
    }
    const float mx = wave_max(s);
    const float p = lane < nk ? __expf(s - mx) : 0.f;        // every key masked: -inf - -inf = NaN, like torch
    const float den = wave_sum(p);
    ps[lane] = p / den;
    __syncthreads();
    const bf16_t* v;
    if constexpr (VL) v = a.v + (size_t)key_off[r] * a.ldkv + h * a.hd;
    else v = a.v + (size_t)r * a.keys_stride * a.ldkv + h * a.hd;
    for (int d = lane; d < a.hd; d += 64) {
        float acc = 0.f;
        for (int i = 0; i < nk; ++i) acc += ps[i] * bf2f(v[(size_t)i * a.ldkv + d]);    // fixed order: batch invariant
        a.ctx[(size_t)m * a.ldc + h * a.hd + d] = f2bf(acc);
    }
}

// attn_small_kernel's cross-attention scores and softmax for one (query, head) -- the same loads, the same order of the products,
// the same butterflies, __expf and division --, written out instead of being multiplied into V: lane i owns memory token (frame) i.
// VL: attn_small_kernel<true>'s keys; the row of probs keeps its a.F columns, those from key_len[r] on hold 0.
template <bool VL>
__global__ __launch_bounds__(64) void cross_probs_kernel(CrossProbsArgs a, const int32_t* __restrict__ key_off, const int32_t* __restrict__ key_len) {
    __shared__ float qs[128];
    const int lane = threadIdx.x, m = blockIdx.x, h = blockIdx.y;
    const int r = m / a.T;
    int nk;
    if constexpr (VL) nk = min(max(key_len[r], 0), a.F);
    else nk = a.F;
    const bf16_t* q = a.q + (size_t)m * a.ldq + h * a.hd;
    for (int d = lane; d < a.hd; d += 64) qs[d] = bf2f(q[d]);
    __syncthreads();
    float s = -INFINITY;
    if (lane < nk) {
        const bf16_t* k;
        if constexpr (VL) k = a.k + (size_t)(key_off[r] + lane) * a.ldkv + h * a.hd;
        else k = a.k + (size_t)(r * a.keys_stride + lane) * a.ldkv + h * a.hd;
        float acc = 0.f;
        for (int c = 0; c < a.hd; c += 8) {
            const bf16x8 kk = *(const bf16x8*)(k + c);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc += qs[c + e] * bf2f((bf16_t)kk[e]);
        }
        s = acc * rsqrtf((float)a.hd);
    }
    const float mx = wave_max(s);
    const float p = lane < nk ? __expf(s - mx) : 0.f;
    const float den = wave_sum(p);
    if constexpr (VL) {
        if (lane < a.F) a.probs[((size_t)m * a.H + h) * a.F + lane] = lane < nk ? p / den : 0.f;
    } else {
        if (lane < a.F) a.probs[((size_t)m * a.H + h) * a.F + lane] = p / den;
    }
}

// one thread per (m, frame): layers, then heads, ascending
__global__ void cross_mean_kernel(const float* __restrict__ probs, int L, int M, int T, int H, int F, int layer, const int32_t* __restrict__ lengths,
                                  float* __restrict__ out, int ld_f) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= M * F) return;
    const int m = i / F, f = i - m * F, r = m / T, j = m - r * T;
    float acc = 0.f;
    if (!lengths || j < lengths[r]) {
        const int l0 = layer < 0 ? 0 : layer, l1 = layer < 0 ? L : layer + 1;
        for (int l = l0; l < l1; ++l)
            for (int h = 0; h < H; ++h) acc += probs[(((size_t)l * M + m) * H + h) * F + f];
        acc = acc / (float)((l1 - l0) * H);
    }
    out[(size_t)m * ld_f + f] = acc;
}

struct StuLayer {
    const bf16_t *sa_in_w, *sa_out_w, *ca_in_w, *ca_out_w, *l1w, *l2w;
    const float *sa_in_b, *sa_out_b, *ca_in_b, *ca_out_b, *l1b, *l2b, *n1w, *n1b, *n2w, *n2b, *n3w, *n3b;
};

}  // namespace

hipError_t launch_attn_small(const SmallAttnArgs& a, hipStream_t s) {
    if (a.M <= 0 || a.H <= 0 || a.hd % 8 || a.hd > 128 || a.nkeys > 64 || (a.nkeys == 0 && a.t0 + a.T > 64)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(attn_small_kernel<false>, dim3(a.M, a.H), dim3(64), 0, s, a, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_attn_small_varlen(const SmallAttnArgs& a, const int32_t* key_off, const int32_t* key_len, hipStream_t s) {
    if (!key_off || !key_len || a.M <= 0 || a.T <= 0 || a.H <= 0 || a.hd <= 0 || a.hd % 8 || a.hd > 128 || a.ids) return hipErrorInvalidValue;
    hipLaunchKernelGGL(attn_small_kernel<true>, dim3(a.M, a.H), dim3(64), 0, s, a, key_off, key_len);
    return hipGetLastError();
}

static bool cross_probs_ok(const CrossProbsArgs& a) {
    return a.q && a.k && a.probs && a.M > 0 && a.T > 0 && a.M % a.T == 0 && a.H > 0 && a.hd > 0 && a.hd % 8 == 0 && a.hd <= 128 && a.F > 0 && a.F <= 64;
}

hipError_t launch_cross_probs(const CrossProbsArgs& a, hipStream_t s) {
    if (!cross_probs_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cross_probs_kernel<false>, dim3(a.M, a.H), dim3(64), 0, s, a, nullptr, nullptr);
    return hipGetLastError();
}

hipError_t launch_cross_probs_varlen(const CrossProbsArgs& a, const int32_t* key_off, const int32_t* key_len, hipStream_t s) {
    if (!key_off || !key_len || !cross_probs_ok(a)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(cross_probs_kernel<true>, dim3(a.M, a.H), dim3(64), 0, s, a, key_off, key_len);
    return hipGetLastError();
}

hipError_t launch_cross_mean(const float* probs, int L, int rows, int T, int H, int F, int layer, const int32_t* lengths,
                             float* frame_mass, int ld_f, hipStream_t s) {
    if (!probs || !frame_mass || L <= 0 || rows <= 0 || T <= 0 || H <= 0 || F <= 0 || layer < -1 || layer >= L || ld_f < F ||
        (int64_t)rows * T * F > 0x7fffffff)
        return hipErrorInvalidValue;
    const int n = rows * T * F;
    hipLaunchKernelGGL(cross_mean_kernel, dim3((n + 255) / 256), dim3(256), 0, s, probs, L, rows * T, T, H, F, layer, lengths, frame_mass, ld_f);
    return hipGetLastError();
}

hipError_t launch_student_embed(const int64_t* ids, int ld_ids, int rows, int T, int t0, const float* embed,
                                const float* pe, int D, int vocab, float* xf, bf16_t* xb, hipStream_t s) {
    if (rows <= 0 || T <= 0 || D % 4) return hipErrorInvalidValue;
    // torch.sqrt(torch.tensor(D)) of model.py:144 in fp32
    hipLaunchKernelGGL(student_embed_kernel, dim3(rows * T), dim3(64), 0, s, ids, ld_ids, T, t0, embed, pe, D, vocab,
                       sqrtf((float)D), xf, xb);
    return hipGetLastError();
}

// ---- device-resident beam search of the student (model.py:189-318): bookkeeping kernels ----------------------------------
// dst[(b * k + i)][:] = src[b][:]  (the k beams of a clip share its memory rows)
__global__ __launch_bounds__(256) void repeat_rows_kernel(const float* __restrict__ src, float* __restrict__ dst, int k, int n4) {
    const int r = blockIdx.y;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < n4; i += gridDim.x * 256)
        ((f32x4*)dst)[(size_t)r * n4 + i] = ((const f32x4*)src)[(size_t)(r / k) * n4 + i];
}
// beam scores before the first step: only beam 0 of every clip is live (all k rows hold the same prefix [CLS])
__global__ void beam_scores_init_kernel(float* scores, int rows, int k) {
    const int r = blockIdx.x * 64 + threadIdx.x;
    if (r < rows) scores[r] = (r % k == 0) ? 0.f : -1e9f;
}
// one step of model.py:252-287: candidate j of clip b (sorted best first by beam_topk; flat index = beam * V + token) becomes
// row b * k + j: its prefix is the prefix of row b * k + beam, its new token the candidate's, its score the candidate's
// FORCED (gitcap_student_attach_prompt; pr indexed by clip, pr.pos = t + 1 = the position written): a clip still inside its prompt
// (t + 1 < len_b) is not ranked -- every one of its k rows keeps its OWN prefix and appends the prompt's token, src_rows is the
// identity, scores stay as they are (a clip leaves its prompt with [0, -1e9, ..], as it leaves CLS) and its candidates are not read.
// <false> is the kernel as it was before it became a template.
template <bool FORCED>
__global__ __launch_bounds__(64) void student_beam_step_kernel(const float* __restrict__ cand_scores, const int* __restrict__ cand_idx,
                                                               const int64_t* __restrict__ ids_cur, int64_t* __restrict__ ids_next,
                                                               float* __restrict__ scores, int32_t* __restrict__ src_rows,
                                                               int k, int V, int t, int ld, PromptSel<FORCED> pr) {
    const int b = blockIdx.x, lane = threadIdx.x;
    if constexpr (FORCED) {
        if (pr.pos < prompt_len(pr.lengths, b, pr.max_len)) {
            const int64_t tok = pr.ids[(size_t)b * pr.ld + pr.pos];
            for (int j = 0; j < k; ++j) {
                const int row = b * k + j;
                for (int i = lane; i <= t; i += 64) ids_next[(size_t)row * ld + i] = ids_cur[(size_t)row * ld + i];
                if (lane == 0) {
                    ids_next[(size_t)row * ld + t + 1] = tok;
                    src_rows[row] = row;
                }
            }
            return;
        }
    }
    for (int j = 0; j < k; ++j) {
        const int idx = cand_idx[b * k + j];
        const int beam = idx / V, tok = idx - beam * V;
        const int src = b * k + beam, dst = b * k + j;
        for (int i = lane; i <= t; i += 64) ids_next[(size_t)dst * ld + i] = ids_cur[(size_t)src * ld + i];
        if (lane == 0) {
            ids_next[(size_t)dst * ld + t + 1] = tok;
            scores[dst] = cand_scores[b * k + j];
            src_rows[dst] = src;
        }
    }
}
// The start of a prompted loop (gitcap_student_attach_prompt), in the place of launch_fill_i64: row r of ids [rows][ld] = CLS, the
// tokens 1 .. len - 1 of prompt row r / k (k beams of a clip share its prompt; k = 1: the greedy loop's rows), CLS in the columns
// behind them (what the fill writes).  len = lengths[r / k] clamped to [1, max_len] (prompt_len: no read leaves a table row).
// lp (nullable, [rows][ld_lp]): its columns 0 .. pmin - 2 become 0.0f, the forced positions a one-pass plan never visits.
// The tables are the handle's and are read when the launch runs: inside a captured loop, at replay.
__global__ __launch_bounds__(64) void student_prompt_stage_kernel(const int64_t* __restrict__ prm_ids, int ld_prm, const int32_t* __restrict__ prm_len,
                                                                  int k, int max_len, int64_t cls, int64_t* __restrict__ ids, int ld,
                                                                  float* __restrict__ lp, int ld_lp, int pmin) {
    const int r = blockIdx.x, c = r / k;
    const int len = prompt_len(prm_len, c, max_len);
    for (int i = threadIdx.x; i < ld; i += 64) ids[(size_t)r * ld + i] = (i >= 1 && i < len) ? prm_ids[(size_t)c * ld_prm + i] : cls;
    if (lp)
        for (int i = threadIdx.x; i + 1 < pmin; i += 64) lp[(size_t)r * ld_lp + i] = 0.0f;
}
// the best beam of every clip (row b * k: the candidates arrive sorted) -> out [B][max_len]
__global__ void student_beam_finish_kernel(const int64_t* __restrict__ ids, int64_t* __restrict__ out, int k, int ld, int max_len) {
    const int b = blockIdx.x;
    for (int i = threadIdx.x; i < max_len; i += 64) out[(size_t)b * max_len + i] = ids[(size_t)b * k * ld + i];
}

// gitcap_student_attach_search's lengths_out: the stored hypotheses' lengths [B][n] by rank, as search.hip's beam_finish_kernel ranks
// the slots (descending score, equal scores in storage order); a rank without a hypothesis holds 0.  One thread per (clip, slot).
__global__ void student_hyp_lengths_kernel(const float* __restrict__ hyp_score, const int32_t* __restrict__ hyp_len, int n, int total,
                                           int32_t* __restrict__ out) {
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= total) return;
    const int b = i / n, slot = i - b * n, len = hyp_len[i];
    int rank = slot;                            // an empty slot: behind every stored one, in slot order
    if (len > 0) {
        rank = 0;
        for (int j = 0; j < n; ++j) {
            if (j == slot || hyp_len[b * n + j] <= 0) continue;
            const float sj = hyp_score[b * n + j];
            rank += sj > hyp_score[i] || (sj == hyp_score[i] && j < slot);
        }
    }
    out[b * n + rank] = len > 0 ? len : 0;
}

hipError_t launch_student_prompt_stage(const StudentPromptStageArgs& a, hipStream_t s) {
    if (!a.prm_ids || !a.prm_len || !a.ids || a.rows < 1 || a.k < 1 || a.max_len < 1 || a.ld_prm < a.max_len || a.ld < a.max_len || a.pmin < 1 ||
        (a.lp && a.ld_lp + 1 < a.pmin))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(student_prompt_stage_kernel, dim3(a.rows), dim3(64), 0, s, a.prm_ids, a.ld_prm, a.prm_len, a.k, a.max_len, a.cls, a.ids, a.ld,
                       a.lp, a.ld_lp, a.pmin);
    return hipGetLastError();
}

hipError_t launch_student_beam_step(const StudentBeamStepArgs& a, hipStream_t s) {
    if (!a.cand_scores || !a.cand_idx || !a.ids_cur || !a.ids_next || !a.scores || !a.src_rows || a.B < 1 || a.k < 1 || a.V < 1 || a.t < 0 ||
        a.ld < a.t + 2)
        return hipErrorInvalidValue;
    const PromptArgs* p = a.prompt;
    if (p && (!p->ids || !p->lengths || p->max_len < 1 || p->ld < p->max_len)) return hipErrorInvalidValue;
    if (p && a.t + 1 < p->max_len)                  // (behind the longest prompt no clip is forced: the plain form)
        hipLaunchKernelGGL(student_beam_step_kernel<true>, dim3(a.B), dim3(64), 0, s, a.cand_scores, a.cand_idx, a.ids_cur, a.ids_next, a.scores,
                           a.src_rows, a.k, a.V, a.t, a.ld, PromptSel<true>{p->ids, p->lengths, p->ld, p->max_len, a.t + 1});
    else
        hipLaunchKernelGGL(student_beam_step_kernel<false>, dim3(a.B), dim3(64), 0, s, a.cand_scores, a.cand_idx, a.ids_cur, a.ids_next, a.scores,
                           a.src_rows, a.k, a.V, a.t, a.ld, PromptSel<false>{});
    return hipGetLastError();
}

// ---- memory-token window (gitcap_student_window_*) -------------------------------------------------------------------------
// push: fp32 tokens [B][n][D] -> bf16 staging rows as two contiguous segments, the n1 tokens per clip that fill the ring up to its
// end ([B][n1][D]) and the n - n1 that wrap to slot 0 ([B][n - n1][D]): each segment is the X of one K|V GEMM whose output rows
// are ring slots (sk_full's T / row_stride / row_off).  f2bf as launch_cast_bf16: the bf16 rows set_memory's GEMM reads.
__global__ __launch_bounds__(256) void student_window_stage_kernel(const float* __restrict__ mem, bf16_t* __restrict__ stage, int B, int n,
                                                                   int n1, int D4) {
    const int64_t total = (int64_t)B * n * D4;
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        const int c = (int)(e % D4), j = (int)((e / D4) % n), b = (int)(e / ((int64_t)D4 * n));
        const int64_t row = j < n1 ? (int64_t)b * n1 + j : (int64_t)B * n1 + (int64_t)b * (n - n1) + (j - n1);
        const f32x4 v = ((const f32x4*)mem)[e];
        uint2 o;
        o.x = pack_bf2(v[0], v[1]);
        o.y = pack_bf2(v[2], v[3]);
        ((uint2*)stage)[row * D4 + c] = o;
    }
}
// window call: K|V rows of the ring [L][B][F slots][2D], oldest slot = head, -> memkv [L][R][F][2D] in window order; decoder row r
// takes clip r / k (k beams per clip share its tokens).  blockIdx.x = (r, f), blockIdx.y = layer; n8 = 2D / 8 16-byte pieces per row.
// n = the tokens copied per row, from slot `head` on: F of a full window, fewer of a partial one (rows keep their pitch of F slots).
__global__ __launch_bounds__(64) void student_window_gather_kernel(const bf16_t* __restrict__ ring, bf16_t* __restrict__ memkv, int F, int head,
                                                                   int k, int n8, size_t ring_layer, size_t mem_layer, int n) {
    const int r = blockIdx.x / n, f = blockIdx.x % n, l = blockIdx.y;
    const uint4* src = (const uint4*)(ring + l * ring_layer) + ((size_t)(r / k) * F + (head + f) % F) * n8;
    uint4* dst = (uint4*)(memkv + l * mem_layer) + ((size_t)r * F + f) * n8;
    for (int i = threadIdx.x; i < n8; i += 64) dst[i] = src[i];
}

// ---- stream pool (gitcap_student_pool_*) ------------------------------------------------------------------------------------
// push: the packed K|V rows of one push, kv [L][cap][2D], -> the pool ring [L][S * F][2D]: row i of every layer goes to ring row
// slot[i] (a table the host validated: stream * F + slot, no row twice).  blockIdx.x = i, blockIdx.y = layer; 16-byte pieces.
__global__ __launch_bounds__(64) void student_pool_scatter_kernel(const bf16_t* __restrict__ kv, bf16_t* __restrict__ ring,
                                                                  const int32_t* __restrict__ slot, int n8, size_t kv_layer, size_t ring_layer) {
    const int i = blockIdx.x, l = blockIdx.y;
    const uint4* src = (const uint4*)(kv + l * kv_layer) + (size_t)i * n8;
    uint4* dst = (uint4*)(ring + l * ring_layer) + (size_t)slot[i] * n8;
    for (int t = threadIdx.x; t < n8; t += 64) dst[t] = src[t];
}
// pool call: decoder row r's tokens, oldest first, -> memkv PACKED (row r starts where row r - 1 ended).  tab [rows][4] = {the
// stream's first ring row, its oldest slot, the tokens it holds n_r, the first memkv row of r}.  blockIdx.x = (r, f), blockIdx.y =
// layer; a block with f >= n_r has nothing to copy.
__global__ __launch_bounds__(64) void student_pool_gather_kernel(const bf16_t* __restrict__ ring, bf16_t* __restrict__ memkv,
                                                                 const int32_t* __restrict__ tab, int F, int n8, size_t ring_layer, size_t mem_layer) {
    const int r = blockIdx.x / F, f = blockIdx.x % F, l = blockIdx.y;
    const int4 t = ((const int4*)tab)[r];
    if (f >= t.z) return;
    const uint4* src = (const uint4*)(ring + l * ring_layer) + ((size_t)t.x + (t.y + f) % F) * n8;
    uint4* dst = (uint4*)(memkv + l * mem_layer) + ((size_t)t.w + f) * n8;
    for (int i = threadIdx.x; i < n8; i += 64) dst[i] = src[i];
}

struct gitcap_student : HandleCore {
    gitcap_student_config c;
    std::map<std::string, DevTensor> w;
    bool finalized = false, have_memory = false;
    int D = 0, H = 0, hd = 0, FF = 0, L = 0, V = 0, F = 0, R = 0, Tmax = 0, Mt = 0, cur_B = 0;
    // workspace: text rows
    float *xf = nullptr, *xf2 = nullptr, *slabs = nullptr, *amax_val = nullptr;
    int* amax_idx = nullptr;
    bf16_t *xb = nullptr, *qc = nullptr, *ctx = nullptr, *ffn = nullptr, *kvs = nullptr, *memb = nullptr, *memkv = nullptr;
    int32_t* sep_cnt = nullptr;
    // the token loops work on the handle's own ids / steps buffers (copy_out: to the caller's); their captured graphs, one entry per
    // key: stop = a stop rule -> execs[0] the whole greedy loop; TAIL_STEPS -> execs[t - 1] token step t of the draft path, t >= 1
    int64_t* g_ids = nullptr;
    int32_t* g_steps = nullptr;
    // tk: top-k alternatives per step (0: none); ragged: the varlen cross-attention launches; cons: the constrained loop; plan: 0 the
    // unprompted loop, 1 a prompted loop of forced token steps, p >= 2 a prompted loop whose positions 0 .. p - 1 run as one pass
    struct Graphs { int B, max_len, stop; bool rows_pro, head_share, lp; int tk; bool ragged, cons; int plan; std::vector<hipGraphExec_t> execs; };
    static constexpr int TAIL_STEPS = -1;
    std::vector<Graphs> graphs;
    // draft verification (gitcap_student_*_greedy_draft): acc_tok / acc_ticket = draft_accept_kernel's scratch, acc_host = its
    // page-locked {accepted, stop rule fired}, read behind acc_ev
    int* acc_tok = nullptr;
    unsigned* acc_ticket = nullptr;
    int32_t* acc_host = nullptr;
    hipEvent_t acc_ev = nullptr;
    StudentOpts pending;        // the one-shot attachments of gitcap_student_attach_* (host_logic.h); entry points take them through take()
    // token log-probabilities (gitcap_student_attach_token_logprobs): the first attach allocates amax_sum (the head's third partial,
    // sized as amax_val), acc_lp (draft_accept_kernel's hand-over words) and g_lp, the handle's own [B][max_len] rows the captured
    // loops write (copied to the caller's buffer behind the replay, like g_ids)
    float *amax_sum = nullptr, *g_lp = nullptr;
    int* acc_lp = nullptr;
    // top-k alternatives (gitcap_student_attach_top_logprobs): the first attach allocates amax_sum and g_tk_ids / g_tk_lp, the
    // handle's own [B][max_len][k] rows the captured loops write (copied out like g_lp)
    int64_t* g_tk_ids = nullptr;
    float* g_tk_lp = nullptr;
    float* score_buf = nullptr;         // gitcap_student_score (first use): [2][Mt] target logits, lp rows the caller did not ask for
    // gitcap_student_attention (first use): att_probs [L][Mt][H][F] cross-attention probabilities; att_on: the pass being issued
    // writes them (one more launch per layer behind the cross-attention q projection), off for every other call
    float* att_probs = nullptr;
    bool att_on = false;
    // clips of different length (gitcap_student_attach_frame_counts): ragged = the memory currently set is packed: memkv holds one
    // K|V row per frame, clip-major, and decoder row r reads rows key_off[r] .. + key_len[r] - 1 of it (key_tab: device int32 [2][R],
    // offsets then lengths; the cross-attention launches of text_forward take the varlen forms).  The tables are written outside the
    // captured loops, from key_host ([2][R]); the loops read them at replay, so one graph serves every set of counts.
    bool ragged = false;
    int32_t* key_tab = nullptr;
    HostStage key_host;
    // constrained decoding (gitcap_student_attach_constraints): the first attach allocates ban_mask (uint16 [R][ban_ld], the step's
    // rows), ban_rec (device int32 [BAN_REC_WORDS]: n, min_length, n_suppress, 0, the ids) and ban_host, the staging of the record's
    // header.  The constrained token loop is a graph of its own whose mask launches read ban_rec when they run: the consuming call
    // writes it outside the graph (write_ban_record), so one captured loop serves every set of rules.
    uint16_t* ban_mask = nullptr;
    int ban_ld = 0;
    int32_t* ban_rec = nullptr;
    HostStage ban_host;
    // prompted decoding (gitcap_student_attach_prompt; the attachment names the caller's device tables): the first attach allocates
    // prm_ids (int64 [R][Tmax + 1]) and prm_len (int32 [R]), the handle's own tables: the consuming call copies the caller's rows
    // into them on its stream, outside every captured loop (write_prompt_tables), and the loops' nodes -- the stage kernel, the
    // forced arg-max -- name only these, so one captured loop serves every prompt of its plan.
    int64_t* prm_ids = nullptr;
    int32_t* prm_len = nullptr;
    int64_t draft_calls = 0, draft_offered = 0, draft_accepted = 0, draft_tail_steps = 0;
    hipStream_t cap_stream = nullptr;   // capture only (the legacy default stream cannot be captured); replays run on the caller's stream
    // device-resident beam search (gitcap_student_beam_search), allocated on first use
    struct BeamWs {
        float *memrep = nullptr, *scores = nullptr, *cand_scores = nullptr, *logits = nullptr;
        int* cand_idx = nullptr; int32_t* src_rows = nullptr;
        int64_t *ids0 = nullptr, *ids1 = nullptr;
        bf16_t* kvs2 = nullptr; char* topk_scratch = nullptr;
        // the search that ends hypotheses at SEP (gitcap_student_attach_search), allocated by its first call: what search.hip's
        // bookkeeping keeps beside the buffers above -- words [R], done / hyp_len / hyp_score [R] (B * n <= B * k), hyp_ids
        // [R][Tmax] -- and candidate slots for k * per_node_beam_size <= 16 per clip ([R][16]: B <= R clips)
        int64_t *words = nullptr, *hyp_ids = nullptr;
        int32_t *done = nullptr, *hyp_len = nullptr;
        float *hyp_score = nullptr, *cand16_scores = nullptr;
        int* cand16_idx = nullptr;
    } bw;
    // memory-token window (gitcap_student_window_*), allocated by window_reset: ring = the cross-attention K|V rows of the last F
    // tokens of win_B clips, bf16 [L][win_B][F slots][2D]; win (RingCursor) = where the next token goes and how many have been
    // pushed per clip; win_order (RingOrder) = a push behind the last window call's gather and the last push, a window call behind
    // the last push.
    bf16_t *win_ring = nullptr, *win_stage = nullptr;
    int win_B = 0;
    RingCursor win;
    RingOrder win_order;
    // stream pool (gitcap_student_pool_*), allocated by pool_reset and state of its own beside the window: pool_ring = the K|V rows
    // of pool_S independent streams, bf16 [L][pool_S][F slots][2D]; pool (one RingCursor per stream) = where a stream's next token
    // goes and how many it holds.  One push: pool_stage = its tokens cast, packed [pool_cap][D]; pool_kv = their K|V rows, packed
    // [L][pool_cap][2D]; pool_slot = the ring row of each (device [pool_cap], staged in pool_slot_host).  One pool call: pool_tab =
    // {ring row base, oldest slot, tokens, first packed memkv row} per decoder row (device [R][4], staged in pool_tab_host).
    // pool_order: win_order's discipline for the pool's ring.
    bf16_t *pool_ring = nullptr, *pool_stage = nullptr, *pool_kv = nullptr;
    int32_t *pool_slot = nullptr, *pool_tab = nullptr;
    HostStage pool_slot_host, pool_tab_host;
    int pool_S = 0, pool_cap = 0;
    int64_t pool_bytes = 0;
    std::vector<RingCursor> pool;
    RingOrder pool_order;
    // resolved weights
    const float *embed = nullptr, *pe = nullptr, *head_b = nullptr;
    const bf16_t* head_w = nullptr;
    std::vector<StuLayer> layers;
};

namespace {

// the captured token loops and token steps: weight pointers are baked into their nodes
void destroy_graphs(gitcap_student* h) {
    for (auto& g : h->graphs)
        for (hipGraphExec_t e : g.execs) (void)hipGraphExecDestroy(e);
    h->graphs.clear();
}

// the stream pool's buffers (the caller has made sure nothing in flight uses them); the events of pool_order stay for the next reset
void pool_free(gitcap_student* h) {
    for (void* p : {(void*)h->pool_ring, (void*)h->pool_stage, (void*)h->pool_kv, (void*)h->pool_slot, (void*)h->pool_tab})
        if (p) (void)hipFree(p);
    h->pool_slot_host.destroy();
    h->pool_tab_host.destroy();
    h->pool_ring = h->pool_stage = h->pool_kv = nullptr;
    h->pool_slot = h->pool_tab = nullptr;
    h->ws_bytes -= h->pool_bytes;
    h->pool_bytes = 0;
    h->pool_S = h->pool_cap = 0;
    h->pool.clear();
}

bool student_is_gemm_weight(const std::string& n) {
    auto ends = [&](const char* s) { size_t l = strlen(s); return n.size() >= l && n.compare(n.size() - l, l, s) == 0; };
    return n == "linear.weight" || ends("in_proj_weight") || ends("out_proj.weight") || ends("linear1.weight") || ends("linear2.weight");
}

// the reference's state_dict keys (gitcap/student_config.py: student_shapes)
void expected_shapes(const gitcap_student_config& c, std::vector<std::pair<std::string, std::vector<int64_t>>>& out) {
    const int64_t D = c.d_model, FF = c.d_ffn, V = c.vocab_size;
    auto add = [&](const std::string& n, std::vector<int64_t> s) { out.emplace_back(n, std::move(s)); };
    add("embed.weight", {V, D});
    add("pos_enc.pe", {1, c.max_pos, D});
    for (int i = 0; i < c.num_layers; ++i) {
        const std::string p = "decoder.layers." + std::to_string(i) + ".";
        for (const char* att : {"self_attn", "multihead_attn"}) {
            add(p + att + ".in_proj_weight", {3 * D, D}); add(p + att + ".in_proj_bias", {3 * D});
            add(p + att + ".out_proj.weight", {D, D}); add(p + att + ".out_proj.bias", {D});
        }
        add(p + "linear1.weight", {FF, D}); add(p + "linear1.bias", {FF});
        add(p + "linear2.weight", {D, FF}); add(p + "linear2.bias", {D});
        for (const char* n : {"norm1", "norm2", "norm3"}) { add(p + n + ".weight", {D}); add(p + n + ".bias", {D}); }
    }
    add("linear.weight", {V, D});
    add("linear.bias", {V});
}

HeadWeight head_weight(const gitcap_student* h) { return HeadWeight{h->head_w, nullptr, nullptr, h->head_b, h->V, h->D}; }

int sk_full(gitcap_student* h, hipStream_t s, int epi, const bf16_t* X, int ldx, const bf16_t* W, const float* bias, int M,
            int N, int K, void* out, int ldo, int T = 1, int row_stride = 1, int row_off = 0) {
    SkinnyArgs a{};
    a.X = X; a.ldx = ldx; a.W = W; a.bias = bias; a.M = M; a.N = N; a.K = K; a.out = out; a.ldo = ldo;
    a.T = T; a.row_stride = row_stride; a.row_off = row_off;
    HIP_OK(h, launch_skinny(a, epi, s));
    return 0;
}

// model.py:128-154 for rows x T query positions t0..t0+T-1 (K/V of earlier positions come from the cache); the request is the
// part the two handles share (RowsReq, kernels.h): logits_out set = the logits of all positions
// ban (nullable; a constrained greedy step): the BAN form of the head, mask row m = head row m
struct TextReq : RowsReq { const HeadBan* ban = nullptr; };
int text_forward(gitcap_student* h, const TextReq& q, hipStream_t s) {
    const gitcap_student_config& c = h->c;
    const int64_t* const ids = q.ids;
    const int ld_ids = q.ld_ids, rows = q.rows, t0 = q.t0, T = q.T;
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "student: weights not finalized");
    if (!h->have_memory) return fail(h, GITCAP_ERR_STATE, "student: decoder called before set_memory");
    if (!ids || rows <= 0 || T <= 0 || t0 < 0) return fail(h, GITCAP_ERR_ARG, "student: bad arguments");
    if (rows != h->cur_B) return fail(h, GITCAP_ERR_ARG, "student: rows != rows of the current memory");
    if (t0 + T > h->Tmax) return fail(h, GITCAP_ERR_ARG, "student: t0+T exceeds max_text_len+1");
    if (t0 + T > c.max_pos) return fail(h, GITCAP_ERR_ARG, "student: position exceeds the positional table");
    const int D = h->D, M = rows * T;
    int rc;
    HIP_OK(h, launch_student_embed(ids, ld_ids, rows, T, t0, h->embed, h->pe, D, h->V, h->xf, h->xb, s));
    const size_t kvs_layer = (size_t)h->R * h->Tmax * 3 * D, mem_layer = (size_t)h->R * h->F * 2 * D;
    // Each post-LN sub-layer is split-K partial slabs -> sum + bias + residual + LayerNorm.  With one or two rows (the webcam
    // case) that row kernel is not launched: the projection that consumes its output computes the rows itself (skinny.hip
    // "row prologue", same code -> same bits) and workgroup 0 writes the fp32 residual rows to the other of two buffers.
    const bool rows_pro = g_row_prologue && skinny_row_prologue_ok(M, D, false);
    float *xcur = h->xf, *xalt = h->xf2;
    struct { bool on; const float *bias, *g, *b; int nslab; } pend{false, nullptr, nullptr, nullptr, 0};
    // out = epi(LN-output . W^T + bias): the LN output is xb, or -- when a reduce + LayerNorm is pending -- computed in place
    auto proj = [&](int epi, const bf16_t* W, const float* bias, int N, void* out, int ldo, int Tq, int row_stride, int row_off) -> int {
        if (!pend.on) return sk_full(h, s, epi, h->xb, D, W, bias, M, N, D, out, ldo, Tq, row_stride, row_off);
        SkinnyArgs a{};
        a.X = h->xb; a.ldx = D; a.W = W; a.bias = bias; a.M = M; a.N = N; a.K = D; a.out = out; a.ldo = ldo;
        a.T = Tq; a.row_stride = row_stride; a.row_off = row_off;
        a.ln.kind = 1; a.ln.slabs = h->slabs; a.ln.nslab = pend.nslab; a.ln.bias = pend.bias; a.ln.resid = xcur;
        a.ln.g = pend.g; a.ln.b = pend.b; a.ln.eps = h->c.ln_eps; a.ln.xf = xalt;
        HIP_OK(h, launch_skinny(a, epi, s));
        std::swap(xcur, xalt);
        pend.on = false;
        return 0;
    };
    // x = LayerNorm(x + X.W^T + bias): split-K partial slabs, then the row kernel now or (defer) inside the next projection
    auto dense_ln = [&](const bf16_t* X, int K, const bf16_t* W, const float* bias, const float* g, const float* b, bool defer) -> int {
        SkinnyArgs a{};
        a.X = X; a.ldx = K; a.W = W; a.M = M; a.N = D; a.K = K; a.out = h->slabs; a.ldo = D; a.T = 1; a.row_stride = 1;
        HIP_OK(h, launch_skinny_splitk(a, s));
        if (rows_pro && defer) { pend = {true, bias, g, b, skinny_ksplit(K)}; return 0; }
        HIP_OK(h, launch_ln_reduce(h->slabs, skinny_ksplit(K), bias, xcur, g, b, h->c.ln_eps, M, D, xcur, h->xb, s));
        return 0;
    };
    for (int l = 0; l < h->L; ++l) {
        const StuLayer& Ly = h->layers[l];
        bf16_t* kv = h->kvs + (size_t)l * kvs_layer;
        // self-attention: q | k | v of the new positions go straight into the cache rows (r, t0 + j)
        if ((rc = proj(SK_BIAS_BF16, Ly.sa_in_w, Ly.sa_in_b, 3 * D, kv, 3 * D, T, h->Tmax, t0))) return rc;
        SmallAttnArgs sa{kv, 3 * D, T, h->Tmax, t0, kv + D, kv + 2 * D, 3 * D, h->Tmax, 0, t0,
                         ids, ld_ids, c.pad_token_id, h->ctx, D, M, h->H, h->hd};
        HIP_OK(h, launch_attn_small(sa, s));
        if ((rc = dense_ln(h->ctx, D, Ly.sa_out_w, Ly.sa_out_b, Ly.n1w, Ly.n1b, true))) return rc;
        // cross-attention over the frame tokens (K/V precomputed by set_memory)
        if ((rc = proj(SK_BIAS_BF16, Ly.ca_in_w, Ly.ca_in_b, D, h->qc, D, 1, 1, 0))) return rc;
        const bf16_t* mkv = h->memkv + (size_t)l * mem_layer;
        SmallAttnArgs ca{h->qc, D, T, T, 0, mkv, mkv + D, 2 * D, h->F, h->F, 0, nullptr, 0, 0, h->ctx, D, M, h->H, h->hd};
        // ragged: the memory rows are packed and row r's keys come through the tables (the varlen forms: same arithmetic)
        const int32_t *key_off = h->key_tab, *key_len = h->ragged ? h->key_tab + h->R : nullptr;
        if (h->att_on) {    // gitcap_student_attention: the probabilities of the launch below, from the q and memory K it reads
            const CrossProbsArgs pa{h->qc, D, T, mkv, 2 * D, h->F, h->F, h->att_probs + (size_t)l * M * h->H * h->F, M, h->H, h->hd};
            HIP_OK(h, h->ragged ? launch_cross_probs_varlen(pa, key_off, key_len, s) : launch_cross_probs(pa, s));
        }
        HIP_OK(h, h->ragged ? launch_attn_small_varlen(ca, key_off, key_len, s) : launch_attn_small(ca, s));
        if ((rc = dense_ln(h->ctx, D, Ly.ca_out_w, Ly.ca_out_b, Ly.n2w, Ly.n2b, true))) return rc;
        // feed-forward (the last layer's LayerNorm is a launch: the vocabulary head reads its bf16 output)
        if ((rc = proj(SK_BIAS_RELU_BF16, Ly.l1w, Ly.l1b, h->FF, h->ffn, h->FF, 1, 1, 0))) return rc;
        if ((rc = dense_ln(h->ffn, h->FF, Ly.l2w, Ly.l2b, Ly.n3w, Ly.n3b, l + 1 < h->L))) return rc;
    }
    if (!q.logits_out && !q.argmax_out && !q.score) return 0;
    if (q.score) {      // gitcap_student_score: all positions, no logits; the three partials + the given tokens' logits -> score_final
        if (!h->amax_sum || !h->score_buf) return fail(h, GITCAP_ERR_STATE, "student: scoring without its buffers");
        HIP_OK(h, launch_score(head_weight(h), h->xb, ids, ld_ids, rows, T, h->amax_val, h->amax_idx, h->amax_sum, h->score_buf, *q.score, s));
        return 0;
    }
    // vocabulary head: all positions when logits are requested, else the last position of every row
    if ((q.lp_out || q.topk.k) && (!q.argmax_out || !h->amax_sum))
        return fail(h, GITCAP_ERR_STATE, "student: token log-probabilities or top-k alternatives without their partials");
    SkinnyArgs ha;
    const HeadRows hr = vocab_head_args(ha, head_weight(h), h->xb, rows, T, q.logits_out != nullptr, q.logits_out,
                                        q.argmax_out ? h->amax_val : nullptr, q.argmax_out ? h->amax_idx : nullptr,
                                        q.lp_out || q.topk.k ? h->amax_sum : nullptr);
    HIP_OK(h, launch_skinny(ha, SK_BIAS_F32, s, nullptr, q.ban));
    if (q.argmax_out) {
        ArgmaxArgs a{};
        a.val = h->amax_val; a.idx = h->amax_idx; a.sum = q.lp_out ? h->amax_sum : nullptr; a.ntiles = (h->V + 15) / 16;
        a.rows = rows; a.row_stride = hr.am_stride; a.row_off = hr.am_off;
        a.out = q.argmax_out; a.ld_out = q.ld_argmax; a.sep_cnt = q.sep_cnt; a.step = q.step; a.sep_id = c.sep_token_id;
        a.lp_out = q.lp_out; a.ld_lp = q.ld_lp;
        a.prompt = q.prompt; a.prompt_pos = t0 + T;         // (a prompted greedy loop): the token goes to position t0 + T
        HIP_OK(h, launch_argmax_final(a, s));
    }
    if (q.topk.k) {     // the k best of the row the arg-max read, from the same partials
        HeadTopkArgs ta{};
        ta.X = ha.X; ta.ldx = ha.ldx; ta.hw = head_weight(h); ta.val = h->amax_val; ta.idx = h->amax_idx; ta.sum = h->amax_sum; ta.bn = q.ban;
        ta.rows = rows; ta.T = 1; ta.row_stride = hr.am_stride; ta.row_off = hr.am_off;
        ta.k = q.topk.k; ta.top_ids = q.topk.ids; ta.top_lp = q.topk.lp; ta.ld = q.topk.ld;
        HIP_OK(h, launch_head_topk(ta, s));
    }
    return 0;
}

// ---- clips of different length (gitcap_student_attach_frame_counts) -------------------------------------------------------------
using Counts = std::vector<int32_t>;
// An entry point's take (host_logic.h: take_opts): the parts in `parts` go to *o, consumed whatever becomes of the call; of the parts in
// `refuse`, cleared, the first that held an attachment is the call's error: counts, prompt, constraints, search options, top-k, as
// ever reported.
int take(gitcap_student* h, const std::string& who, unsigned parts, unsigned refuse, StudentOpts* o = nullptr) {
    unsigned refused = 0;
    StudentOpts taken = take_opts(h->pending, parts, refuse, &refused);
    if (o) *o = std::move(taken);
    const char* what = refused & OPT_FC ? ": per-clip frame counts are attached (gitcap_student_attach_frame_counts), which this call does not take"
                     : refused & OPT_PR ? ": a prompt is attached (gitcap_student_attach_prompt), which a draft call does not take"
                     : refused & OPT_CO ? ": constraints are attached (gitcap_student_attach_constraints), which a draft call does not take"
                     : refused & OPT_SO ? ": search options are attached (gitcap_student_attach_search), which only the beam family takes" : nullptr;
    if (what) return fail(h, GITCAP_ERR_ARG, who + what);
    return refused & OPT_TK ? fail(h, GITCAP_ERR_ARG, refused_message(who.c_str(), OPT_TK)) : 0;
}
// Decoder rows 0 .. rows - 1 read the packed memory rows off(r) .. off(r) + len(r) - 1: the two device tables, written on `s`
// (outside every captured loop).
template <typename Row>
int write_key_tables(gitcap_student* h, int rows, Row row, hipStream_t s) {
    if (rows < 1 || rows > h->R) return fail(h, GITCAP_ERR_ARG, "student: rows outside [1, max_rows]");
    HIP_OK(h, h->key_host.ensure(2 * (size_t)h->R));
    if (!h->key_tab) {
        if (int rc = dev_alloc(h, &h->key_tab, 2 * (size_t)h->R)) { h->key_tab = nullptr; return rc; }
    }
    HIP_OK(h, h->key_host.wait());
    for (int r = 0; r < rows; ++r) {
        const std::pair<int, int> ol = row(r);
        h->key_host.p[r] = ol.first;
        h->key_host.p[h->R + r] = ol.second;
    }
    HIP_OK(h, h->key_host.copy(h->key_tab, 0, (size_t)rows, s));
    HIP_OK(h, h->key_host.copy(h->key_tab + h->R, (size_t)h->R, (size_t)rows, s));
    HIP_OK(h, h->key_host.mark(s));
    return 0;
}

// fc (non-null, not all mem_tokens): memory is the packed [sum(fc)][D] rows of B = fc.size() clips, and the k rows b * k .. b * k + k - 1
// share clip b's K|V rows through the tables.  Otherwise memory is [B][mem_tokens][D], one clip per row.
int set_memory(gitcap_student* h, const float* memory, int B, hipStream_t s, const Counts* fc = nullptr, int k = 1) {
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "student: weights not finalized");
    if (!memory || B <= 0 || k <= 0 || (int64_t)B * k > h->R) return fail(h, GITCAP_ERR_ARG, "student: set_memory: bad arguments / B exceeds max_rows");
    const int D = h->D;
    int Mm = B * h->F;
    if (fc) {
        Counts off(B);
        Mm = 0;
        for (int b = 0; b < B; ++b) { off[b] = Mm; Mm += (*fc)[b]; }
        if (int rc = write_key_tables(h, B * k, [&](int r) { return std::make_pair((int)off[r / k], (int)(*fc)[r / k]); }, s)) return rc;
    }
    h->ragged = fc != nullptr;
    HIP_OK(h, launch_cast_bf16(memory, h->memb, (int64_t)Mm * D, s));
    const size_t mem_layer = (size_t)h->R * h->F * 2 * D;
    for (int l = 0; l < h->L; ++l) {
        const StuLayer& Ly = h->layers[l];
        // k | v = memory . W[D:3D]^T + b[D:3D]   (rows D..3D of the cross-attention in_proj)
        int rc = sk_full(h, s, SK_BIAS_BF16, h->memb, D, Ly.ca_in_w + (size_t)D * D, Ly.ca_in_b + D, Mm, 2 * D, D,
                         h->memkv + (size_t)l * mem_layer, 2 * D);
        if (rc) return rc;
    }
    h->cur_B = B * k;
    h->have_memory = true;
    return 0;
}
// The counts a memory-taking entry point took -> what set_memory gets: null for none and for all-mem_tokens counts (today's dense
// path, launch for launch), else the counts; a B that is not theirs is refused.
int counts_for_call(gitcap_student* h, const std::string& who, const Counts& fc, int B, const Counts** out) {
    *out = nullptr;
    if (fc.empty()) return 0;
    if ((int)fc.size() != B)
        return fail(h, GITCAP_ERR_ARG, who + ": B = " + std::to_string(B) + ", but frame counts of " + std::to_string(fc.size()) + " clips are attached");
    if (!std::all_of(fc.begin(), fc.end(), [&](int32_t c) { return c == h->F; })) *out = &fc;
    return 0;
}

}  // namespace

// ---- student_internal.h: what gitcap_distill (gitcap.hip) needs of this handle ----------------------------------------------------
int student_device(const gitcap_student* h) { return h->device; }
HeadWeight student_head_weight(const gitcap_student* h) { return head_weight(h); }
int student_rows_check(const gitcap_student* h, int rows, int T, std::string& why) {
    auto no = [&](int code, const char* m) { why = m; return code; };
    if (!h->finalized) return no(GITCAP_ERR_STATE, "student: weights not finalized");
    if (!h->have_memory) return no(GITCAP_ERR_STATE, "student: decoder called before set_memory");
    if (rows <= 0 || T <= 0) return no(GITCAP_ERR_ARG, "student: bad arguments");
    if (rows != h->cur_B) return no(GITCAP_ERR_ARG, "student: rows != rows of the current memory");
    if (T > h->Tmax) return no(GITCAP_ERR_ARG, "student: T exceeds max_text_len+1");
    if (T > h->c.max_pos) return no(GITCAP_ERR_ARG, "student: position exceeds the positional table");
    return 0;
}
int student_forward_rows(gitcap_student* h, const int64_t* ids, int ld_ids, int rows, int T, hipStream_t s, StudentRows* out, std::string& why) {
    TextReq q;                  // the stack's rows only, no head
    q.ids = ids; q.ld_ids = ld_ids; q.rows = rows; q.T = T;
    const int rc = text_forward(h, q, s);
    if (rc) { why = h->err; return rc; }
    *out = StudentRows{h->xb, head_weight(h)};
    return 0;
}

extern "C" {

const char* gitcap_student_last_error(const gitcap_student_t* h) { return h ? h->err.c_str() : create_err<gitcap_student>().c_str(); }

int gitcap_student_create(const gitcap_student_config* cfg, int device, gitcap_student_t** out) {
    if (!cfg || !out) return fail<gitcap_student>(nullptr, GITCAP_ERR_ARG, "student_create: null argument");
    const gitcap_student_config& c = *cfg;
    if (c.d_model <= 0 || c.n_head <= 0 || c.d_model % c.n_head || c.d_model % 32 || c.d_ffn % 32 || c.d_model > 1024)
        return fail<gitcap_student>(nullptr, GITCAP_ERR_ARG, "student_create: d_model/d_ffn must be multiples of 32, d_model <= 1024 and divisible by n_head");
    const int hd = c.d_model / c.n_head;
    if (hd % 8 || hd > 128) return fail<gitcap_student>(nullptr, GITCAP_ERR_ARG, "student_create: head_dim must be a multiple of 8, <= 128");
    if (!skinny_full_ok(c.d_model) || !skinny_ksplit(c.d_model) || !skinny_ksplit(c.d_ffn))
        return fail<gitcap_student>(nullptr, GITCAP_ERR_ARG, "student_create: no skinny-GEMM instantiation for this d_model / d_ffn (d_model in {64,128,256,576,768,1024})");
    if (c.num_layers <= 0 || c.vocab_size <= 0 || c.mem_tokens <= 0 || c.mem_tokens > 64 || c.max_rows <= 0)
        return fail<gitcap_student>(nullptr, GITCAP_ERR_ARG, "student_create: bad layer / vocabulary / memory sizes (mem_tokens <= 64)");
    if (c.max_text_len <= 0 || c.max_text_len + 1 > 64 || c.max_text_len + 1 > c.max_pos)
        return fail<gitcap_student>(nullptr, GITCAP_ERR_ARG, "student_create: max_text_len must be in 1..63 and fit the positional table");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || device < 0 || device >= ndev)
        return fail<gitcap_student>(nullptr, GITCAP_ERR_HIP, "student_create: no such HIP device (libgitcap has no CPU fallback)");
    gitcap_student* h = new gitcap_student();
    h->c = c; h->device = device;
    h->D = c.d_model; h->H = c.n_head; h->hd = hd; h->FF = c.d_ffn; h->L = c.num_layers; h->V = c.vocab_size;
    h->F = c.mem_tokens; h->R = c.max_rows; h->Tmax = c.max_text_len + 1; h->Mt = h->R * h->Tmax;
    std::vector<std::pair<std::string, std::vector<int64_t>>> shapes;
    expected_shapes(c, shapes);
    for (auto& kv : shapes) {
        DevTensor t;
        t.shape = kv.second;
        t.kind = student_is_gemm_weight(kv.first) ? 1 : 0;
        h->w[kv.first] = t;
    }
    *out = h;
    return 0;
}

void gitcap_student_destroy(gitcap_student_t* h) {
    if (!h) return;
    DeviceGuard g(h->device);
    for (auto& kv : h->w)
        if (kv.second.p) (void)hipFree(kv.second.p);
    destroy_graphs(h);
    if (h->cap_stream) (void)hipStreamDestroy(h->cap_stream);
    if (h->acc_host) (void)hipHostFree(h->acc_host);
    if (h->acc_ev) (void)hipEventDestroy(h->acc_ev);
    h->key_host.destroy();
    h->ban_host.destroy();
    free_allocs(*h);
    if (h->win_ring) (void)hipFree(h->win_ring);
    if (h->win_stage) (void)hipFree(h->win_stage);
    h->win_order.destroy();
    pool_free(h);
    h->pool_order.destroy();
    delete h;
}

int gitcap_student_load_tensor(gitcap_student_t* h, const char* name, const float* data, const int64_t* shape, int rank) {
    if (!h || !name || !data || !shape) return fail(h, GITCAP_ERR_ARG, "student_load_tensor: null argument");
    std::string why;
    DevTensor* tp = find_tensor(h->w, name, shape, rank, "student_load_tensor", why);
    if (!tp) return fail(h, GITCAP_ERR_ARG, why);
    GUARD(h);
    DevTensor& t = *tp;
    int64_t rows = 1;
    for (int i = 0; i + 1 < rank; ++i) rows *= shape[i];
    const int64_t cols = shape[rank - 1];
    if (t.p) { (void)hipFree(t.p); t.p = nullptr; }
    if (t.kind == 1) {   // GEMM weights: bf16, rows padded to 16 (zero rows)
        if (int rc = upload_bf16_panel(h, t, data, rows, cols, 16, cols)) return rc;
    } else {
        const size_t bytes = (size_t)rows * cols * 4;
        HIP_OK(h, hipMalloc(&t.p, bytes));
        HIP_OK(h, hipMemcpy(t.p, data, bytes, hipMemcpyHostToDevice));
    }
    t.loaded = true;
    h->finalized = false;
    return 0;
}

int gitcap_student_finalize(gitcap_student_t* h) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "student_finalize: null handle");
    GUARD(h);
    for (auto& kv : h->w)
        if (!kv.second.loaded) return fail(h, GITCAP_ERR_STATE, "student_finalize: tensor '" + kv.first + "' was never loaded");
    auto Fp = [&](const std::string& n) { return (const float*)h->w[n].p; };
    auto Wt = [&](const std::string& n) { return (const bf16_t*)h->w[n].p; };
    destroy_graphs(h);
    if (h->pool_ring) {         // the pool's K|V rows came from the weights being replaced: the pool goes, as at pool_reset(0)
        HIP_OK(h, hipDeviceSynchronize());
        pool_free(h);
    }
    h->embed = Fp("embed.weight"); h->pe = Fp("pos_enc.pe"); h->head_w = Wt("linear.weight"); h->head_b = Fp("linear.bias");
    h->layers.resize(h->L);
    for (int i = 0; i < h->L; ++i) {
        const std::string p = "decoder.layers." + std::to_string(i) + ".";
        StuLayer& Ly = h->layers[i];
        Ly.sa_in_w = Wt(p + "self_attn.in_proj_weight"); Ly.sa_in_b = Fp(p + "self_attn.in_proj_bias");
        Ly.sa_out_w = Wt(p + "self_attn.out_proj.weight"); Ly.sa_out_b = Fp(p + "self_attn.out_proj.bias");
        Ly.ca_in_w = Wt(p + "multihead_attn.in_proj_weight"); Ly.ca_in_b = Fp(p + "multihead_attn.in_proj_bias");
        Ly.ca_out_w = Wt(p + "multihead_attn.out_proj.weight"); Ly.ca_out_b = Fp(p + "multihead_attn.out_proj.bias");
        Ly.l1w = Wt(p + "linear1.weight"); Ly.l1b = Fp(p + "linear1.bias");
        Ly.l2w = Wt(p + "linear2.weight"); Ly.l2b = Fp(p + "linear2.bias");
        Ly.n1w = Fp(p + "norm1.weight"); Ly.n1b = Fp(p + "norm1.bias");
        Ly.n2w = Fp(p + "norm2.weight"); Ly.n2b = Fp(p + "norm2.bias");
        Ly.n3w = Fp(p + "norm3.weight"); Ly.n3b = Fp(p + "norm3.bias");
    }
    if (h->allocs.empty()) {
        const size_t Mt = (size_t)h->Mt, D = (size_t)h->D;
        const int ks = std::max(skinny_ksplit(h->D), skinny_ksplit(h->FF));
        const size_t ntiles = ((size_t)h->V + 15) / 16;
        int rc;
        if ((rc = dev_alloc(h, &h->xf2, 2 * D)) || (rc = dev_alloc(h, &h->xf, Mt * D)) || (rc = dev_alloc(h, &h->xb, Mt * D)) || (rc = dev_alloc(h, &h->qc, Mt * D)) ||
            (rc = dev_alloc(h, &h->ctx, Mt * D)) || (rc = dev_alloc(h, &h->ffn, Mt * h->FF)) ||
            (rc = dev_alloc(h, &h->slabs, (size_t)ks * Mt * D)) || (rc = dev_alloc(h, &h->amax_val, Mt * ntiles)) ||
            (rc = dev_alloc(h, &h->amax_idx, Mt * ntiles)) || (rc = dev_alloc(h, &h->kvs, (size_t)h->L * Mt * 3 * D)) ||
            (rc = dev_alloc(h, &h->memb, (size_t)h->R * h->F * D)) ||
            (rc = dev_alloc(h, &h->memkv, (size_t)h->L * h->R * h->F * 2 * D)) || (rc = dev_alloc(h, &h->sep_cnt, (size_t)h->Tmax + 1)) ||
            (rc = dev_alloc(h, &h->g_ids, (size_t)h->R * h->Tmax)) || (rc = dev_alloc(h, &h->g_steps, (size_t)1)) ||
            (rc = dev_alloc(h, &h->acc_tok, Mt)) || (rc = dev_alloc(h, &h->acc_ticket, (size_t)4)))
            return rc;
    }
    h->finalized = true;
    return 0;
}

int gitcap_student_set_memory(gitcap_student_t* h, const float* memory, int B, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "student_set_memory: null handle");
    StudentOpts o;
    (void)take(h, "student_set_memory", OPT_FC, 0, &o);
    const Counts* ragged = nullptr;
    if (int bad = counts_for_call(h, "student_set_memory", o.fc, B, &ragged)) return bad;
    GUARD(h);
    return set_memory(h, memory, B, (hipStream_t)stream, ragged);
}

int gitcap_student_attach_frame_counts(gitcap_student_t* h, const int32_t* counts, int B) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "student_attach_frame_counts: null handle");
    h->pending.fc.clear();
    if (!counts) return 0;                                   // detach
    if (B < 1 || B > h->R) return fail(h, GITCAP_ERR_ARG, "student_attach_frame_counts: B outside [1, max_rows]");
    for (int b = 0; b < B; ++b)
        if (counts[b] < 1 || counts[b] > h->F)
            return fail(h, GITCAP_ERR_ARG, "student_attach_frame_counts: clip " + std::to_string(b) + " has " + std::to_string(counts[b]) +
                        " frames, outside [1, " + std::to_string(h->F) + "]");
    h->pending.fc.assign(counts, counts + B);
    return 0;
}

int gitcap_student_forward_decoder(gitcap_student_t* h, const int64_t* ids, int ld_ids, int B, int T, float* logits, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "student_forward_decoder: null handle");
    if (!logits) return fail(h, GITCAP_ERR_ARG, "student_forward_decoder: null logits");
    GUARD(h);
    TextReq q;
    q.ids = ids; q.ld_ids = ld_ids; q.rows = B; q.T = T; q.logits_out = logits;
    return text_forward(h, q, (hipStream_t)stream);
}

}  // extern "C"

namespace {

// The token loops are launch-latency bound (26 kernels per token): they are captured and replayed.  GITCAP_STUDENT_GRAPH=0
// launches them kernel by kernel (same kernels, same results).
const bool g_use_graph = !(getenv("GITCAP_STUDENT_GRAPH") && atoi(getenv("GITCAP_STUDENT_GRAPH")) == 0);

// Token step t of the greedy loop (model.py:173-182) on the handle's id rows: position t in, the arg-max as token t + 1 (and, with
// want_lp, its log-probability as column t of g_lp; with tk != 0 the tk best of that distribution as entry t of g_tk_ids / g_tk_lp).
// The full loop, the captured tail steps and the un-graphed tail are this call.
// cons: first the rows' ban mask from the ids so far (prefix 0 .. t) under the rules in ban_rec, then the BAN form of the head.
// prompt (the handle's tables): a row whose prompt covers position t + 1 takes the prompt's token there (the forced arg-max).
int token_step(gitcap_student* h, int B, int t, int max_len, bool want_lp, hipStream_t q, int tk = 0, bool cons = false, const PromptArgs* prompt = nullptr) {
    const int ld = max_len + 1;
    const HeadBan bn{h->ban_mask, h->ban_ld};
    TextReq r;
    if (cons) {
        HIP_OK(h, launch_ban_mask_rec(h->g_ids, ld, B, t + 1, h->c.sep_token_id, h->ban_rec, h->V, h->ban_mask, h->ban_ld, q));
        r.ban = &bn;
    }
    r.ids = h->g_ids; r.ld_ids = ld; r.rows = B; r.t0 = r.step = t; r.T = 1;
    r.argmax_out = h->g_ids + t + 1; r.ld_argmax = ld; r.sep_cnt = h->sep_cnt;
    r.lp_out = want_lp ? h->g_lp + t : nullptr; r.ld_lp = max_len;
    if (tk) r.topk = TopkAttach{tk, h->g_tk_ids + (size_t)t * tk, h->g_tk_lp + (size_t)t * tk, max_len};
    r.prompt = prompt;
    return text_forward(h, r, q);
}

// ---- constrained decoding (gitcap_student_attach_constraints) --------------------------------------------------------------------
// A call whose rows could lose every column is refused: each step bans at most n_suppress listed ids, one id per prefix position and
// SEP; need = the columns the call must still find (1: the arg-max; k: the candidates a clip's ranking keeps).
int cons_check(gitcap_student* h, const std::string& who, const ConsOpt& co, int max_len, int need) {
    if (co.on && (int64_t)co.n_suppress + max_len + need > h->V)
        return fail(h, GITCAP_ERR_ARG, who + ": the attached constraints could ban every column of a row (n_suppress + max_len" +
                    (need > 1 ? " + k > vocab_size)" : " >= vocab_size)"));
    return 0;
}
// The rules of the call -> ban_rec, on `s` and outside every captured loop: the header through its staging, the list by a
// device-to-device copy of the caller's `suppress`.
int write_ban_record(gitcap_student* h, const ConsOpt& co, hipStream_t s) {
    HIP_OK(h, h->ban_host.wait());
    h->ban_host.p[0] = co.ngram; h->ban_host.p[1] = co.min_length; h->ban_host.p[2] = co.n_suppress; h->ban_host.p[3] = 0;
    HIP_OK(h, h->ban_host.copy(h->ban_rec, 0, BAN_REC_HEADER, s));
    HIP_OK(h, h->ban_host.mark(s));
    if (co.n_suppress)
        HIP_OK(h, hipMemcpyAsync(h->ban_rec + BAN_REC_HEADER, co.suppress, (size_t)co.n_suppress * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return 0;
}

// ---- prompted decoding (gitcap_student_attach_prompt) ---------------------------------------------------------------------------
// The caller's prompts of `rows` clips -> the handle's tables, on `s` and outside every captured loop: pr.max_len columns of every row
// and the lengths, device to device (the caller's buffers are read when these copies run, ahead of the loop on the same stream).
int write_prompt_tables(gitcap_student* h, const PromptArgs& pr, int rows, hipStream_t s) {
    HIP_OK(h, hipMemcpy2DAsync(h->prm_ids, ((size_t)h->Tmax + 1) * sizeof(int64_t), pr.ids, (size_t)pr.ld * sizeof(int64_t),
                               (size_t)pr.max_len * sizeof(int64_t), (size_t)rows, hipMemcpyDeviceToDevice, s));
    HIP_OK(h, hipMemcpyAsync(h->prm_len, pr.lengths, (size_t)rows * sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    return 0;
}
// the handle's tables as the forced launches take them: lengths are clamped to the CALL's max_len (>= the prompt's), which fits a
// table row (ld = Tmax + 1)
PromptArgs table_prompt(const gitcap_student* h, const PromptArgs& pr, int call_max_len) {
    return PromptArgs{h->prm_ids, h->Tmax + 1, h->prm_len, pr.min_len, call_max_len};
}

// What enqueue(cap_stream) launches -> one executable graph (replayed on the caller's stream).  A failed enqueue still ends the
// capture and its own status is returned; whatever fails, the hipGraph_t is destroyed and *exec stays null.
template <typename Enqueue>
int capture(gitcap_student* h, const char* what, Enqueue enqueue, hipGraphExec_t* exec) {
    *exec = nullptr;
    if (!h->cap_stream) HIP_OK(h, hipStreamCreateWithFlags(&h->cap_stream, hipStreamNonBlocking));
    hipGraph_t graph = nullptr;
    int rc = 0;
    hipError_t e = hipStreamBeginCapture(h->cap_stream, hipStreamCaptureModeThreadLocal);
    if (e == hipSuccess) {
        rc = enqueue(h->cap_stream);
        e = hipStreamEndCapture(h->cap_stream, &graph);
    }
    if (!rc && e == hipSuccess) e = hipGraphInstantiate(exec, graph, nullptr, nullptr, 0);
    if (graph) (void)hipGraphDestroy(graph);
    if (!rc && e != hipSuccess) rc = fail(h, GITCAP_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return rc;
}

// The executables of a key, captured by fill(execs) at the key's first use; a failed fill caches nothing.  Weight and workspace
// pointers are baked into the nodes (destroy_graphs at every finalize).
template <typename Fill>
int captured_graphs(gitcap_student* h, int B, int max_len, int stop, bool want_lp, int tk, bool cons, int plan, Fill fill, const std::vector<hipGraphExec_t>** out) {
    for (auto& g : h->graphs)
        if (g.B == B && g.max_len == max_len && g.stop == stop && g.rows_pro == g_row_prologue && g.head_share == g_head_share && g.lp == want_lp && g.tk == tk &&
            g.ragged == h->ragged && g.cons == cons && g.plan == plan) {
            *out = &g.execs;
            return 0;
        }
    gitcap_student::Graphs g{B, max_len, stop, g_row_prologue, g_head_share, want_lp, tk, h->ragged, cons, plan, {}};
    if (int rc = fill(g.execs)) {
        for (hipGraphExec_t e : g.execs) (void)hipGraphExecDestroy(e);
        return rc;
    }
    h->graphs.push_back(std::move(g));
    *out = &h->graphs.back().execs;
    return 0;
}

// the handle's ids [B][max_len + 1], steps and (lp.p set) log-probabilities [B][max_len] -> the caller's buffers; the columns of
// lp.p behind max_len (row pitch lp.ld) are not touched
int copy_out(gitcap_student* h, int B, int max_len, int64_t* ids_out, int32_t* steps_out, const LpAttach& lp, hipStream_t s,
             const TopkAttach& tk = TopkAttach{}) {
    if (tk.k) {         // [B][max_len][k] -> the caller's [B][tk.ld][k]; the positions behind max_len are not touched
        const size_t w = (size_t)max_len * tk.k;
        HIP_OK(h, hipMemcpy2DAsync(tk.ids, (size_t)tk.ld * tk.k * 8, h->g_tk_ids, w * 8, w * 8, (size_t)B, hipMemcpyDeviceToDevice, s));
        HIP_OK(h, hipMemcpy2DAsync(tk.lp, (size_t)tk.ld * tk.k * 4, h->g_tk_lp, w * 4, w * 4, (size_t)B, hipMemcpyDeviceToDevice, s));
    }
    HIP_OK(h, hipMemcpyAsync(ids_out, h->g_ids, (size_t)B * (max_len + 1) * sizeof(int64_t), hipMemcpyDeviceToDevice, s));
    if (steps_out) HIP_OK(h, hipMemcpyAsync(steps_out, h->g_steps, sizeof(int32_t), hipMemcpyDeviceToDevice, s));
    if (lp.p)
        HIP_OK(h, hipMemcpy2DAsync(lp.p, (size_t)lp.ld * 4, h->g_lp, (size_t)max_len * 4, (size_t)max_len * 4, (size_t)B, hipMemcpyDeviceToDevice, s));
    return 0;
}

// the token loop of greedy_decode (model.py:171-184) against the memory K|V in h->memkv (set_memory, or the window's gather)
// lp.p set: the loop with token log-probabilities (a graph of its own; column t of g_lp = step t's)
// co.on: the constrained loop (a graph of its own, whatever the rules: they are written to ban_rec here, ahead of the replay)
// pr.ids set: the prompted loop (graphs of their own, one per plan, whatever the prompts: they are copied to the handle's tables here,
// ahead of the replay).  The stage kernel puts every row's prompt into g_ids before the first position runs -- the self-attention masks
// PAD keys by id --, and every step runs the forced arg-max against the tables: the device lengths decide row by row.  Positions
// 0 .. pmin - 1 are prompt in every row: where pmin >= 2 they run as ONE pass (T = pmin, the head on its last position, the arg-max
// forced at position pmin), except under constraints or top-k alternatives, which need every position's step.
int greedy_loop(gitcap_student* h, int B, int max_len, int stop, int64_t* ids_out, int32_t* steps_out, hipStream_t s, const LpAttach& lp,
                const TopkAttach& tk, const ConsOpt& co, const PromptArgs& pr) {
    const bool want_lp = lp.p != nullptr;
    int rc;
    if (co.on && (rc = write_ban_record(h, co, s))) return rc;
    int plan = 0;
    if (pr.ids) {
        std::string why;
        plan = g_prompt_prefill && pr.min_len >= 2 && !co.on && !tk.k && student_rows_check(h, B, pr.min_len, why) == 0 ? pr.min_len : 1;
        if ((rc = write_prompt_tables(h, pr, B, s))) return rc;
    }
    const PromptArgs tab = table_prompt(h, pr, max_len);
    const PromptArgs* const prompt = plan ? &tab : nullptr;
    auto enqueue_loop = [&](hipStream_t q) -> int {
        if (plan) {
            const StudentPromptStageArgs sa{h->prm_ids, h->Tmax + 1, h->prm_len, B, 1, max_len, h->c.cls_token_id, h->g_ids, max_len + 1,
                                            want_lp ? h->g_lp : nullptr, max_len, plan};
            HIP_OK(h, launch_student_prompt_stage(sa, q));
        } else {
            HIP_OK(h, launch_fill_i64(h->g_ids, max_len + 1, B, h->c.cls_token_id, q));    // model.py:171
        }
        HIP_OK(h, hipMemsetAsync(h->sep_cnt, 0, ((size_t)h->Tmax + 1) * 4, q));
        if (plan >= 2) {                            // positions 0 .. plan - 1 in one pass: its arg-max is step plan - 1's
            TextReq r;
            r.ids = h->g_ids; r.ld_ids = max_len + 1; r.rows = B; r.t0 = 0; r.T = plan; r.step = plan - 1;
            r.argmax_out = h->g_ids + plan; r.ld_argmax = max_len + 1; r.sep_cnt = h->sep_cnt;
            r.lp_out = want_lp ? h->g_lp + (plan - 1) : nullptr; r.ld_lp = max_len;
            r.prompt = prompt;
            if (int e = text_forward(h, r, q)) return e;
        }
        for (int t = plan >= 2 ? plan : 0; t < max_len; ++t)                                 // model.py:173-182
            if (int r = token_step(h, B, t, max_len, want_lp, q, tk.k, co.on, prompt)) return r;
        HIP_OK(h, launch_finish_steps(h->sep_cnt, B, max_len, stop, h->g_steps, q));       // model.py:184
        return 0;
    };
    if (g_use_graph) {
        const std::vector<hipGraphExec_t>* loop = nullptr;
        rc = captured_graphs(h, B, max_len, stop, want_lp, tk.k, co.on, plan, [&](std::vector<hipGraphExec_t>& execs) {
            execs.push_back(nullptr);
            return capture(h, "student greedy: capturing the token loop", enqueue_loop, &execs.back());
        }, &loop);
        if (rc) return rc;
        HIP_OK(h, hipGraphLaunch((*loop)[0], s));
    } else if ((rc = enqueue_loop(s))) {
        return rc;
    }
    return copy_out(h, B, max_len, ids_out, steps_out, lp, s, tk);
}

// ---- greedy decoding that verifies a draft caption ------------------------------------------------------------------------
// The cached token loop equals one teacher-forced pass over its own output bit for bit, and a row's result does not depend on the
// rows beside it (tests/test_student.py: test_gpu_greedy_kv_cache_and_token_parity, test_gpu_student_batch_invariance_and_determinism).  So the tokens the loop would emit after
// CLS, d_1, .., d_j are the head's arg-max at position j of ONE pass over the draft (T = n, the launches of one token step), and
// every leading draft token that equals it is a token the loop would have produced: accepted, together with the K/V rows the pass
// wrote for its position.  The first position that differs holds the loop's own token (the corrected one).  The steps behind it
// are the loop's own launches, token_step(t).

// verify -> accept -> tail against the memory K|V in h->memkv; same results as greedy_loop(B, max_len, stop)
int greedy_draft_core(gitcap_student* h, int B, const int64_t* draft, int ld_draft, int n, int max_len, int stop, int64_t* ids_out,
                      int32_t* steps_out, int32_t* accepted_out, hipStream_t s, const LpAttach& lp) {
    int rc;
    const int ld = max_len + 1;
    const bool want_lp = lp.p != nullptr;
    if (!h->acc_host) {
        HIP_OK(h, hipHostMalloc((void**)&h->acc_host, 16, hipHostMallocMapped));
        HIP_OK(h, hipEventCreateWithFlags(&h->acc_ev, hipEventDisableTiming));
    }
    // every token step this key can need is captured now: how many of them run depends on the data, a capture must not
    const std::vector<hipGraphExec_t>* steps = nullptr;
    if (g_use_graph) {
        rc = captured_graphs(h, B, max_len, gitcap_student::TAIL_STEPS, want_lp, 0, false, 0, [&](std::vector<hipGraphExec_t>& execs) {
            for (int t = 1; t < max_len; ++t) {
                execs.push_back(nullptr);
                if (int r = capture(h, "student draft: capturing a token step", [&](hipStream_t q) { return token_step(h, B, t, max_len, want_lp, q); },
                                    &execs.back())) { execs.pop_back(); return r; }
            }
            return 0;
        }, &steps);
        if (rc) return rc;
    }
    // 1. verify: one pass over positions 0 .. n-1 of the staged draft (K/V rows of those positions -> the cache), then the
    //    vocabulary head over all B * n rows, arg-max partials only.  Staging (select.hip: draft_stage_kernel) leaves an id outside
    //    [0, vocab) as -1: the embedding clamps it to a table row, it equals no PAD key and no arg-max, so it can only be rejected.
    //    greedy_entry has checked what the launcher checks: 1 <= n <= max_len (ld = max_len + 1), ld_draft >= n + 1, 1 <= B <= max_rows.
    HIP_OK(h, launch_draft_stage(draft, ld_draft, n, B, h->V, (int64_t)h->c.cls_token_id, h->g_ids, ld, s));
    HIP_OK(h, hipMemsetAsync(h->sep_cnt, 0, ((size_t)h->Tmax + 1) * 4, s));
    TextReq q;
    q.ids = h->g_ids; q.ld_ids = ld; q.rows = B; q.T = n;
    if ((rc = text_forward(h, q, s))) return rc;
    const int ntiles = (h->V + 15) / 16;
    SkinnyArgs ha;      // want_lp: the covered positions' log-probabilities come from this pass (the same bits as the loop's)
    vocab_head_args(ha, head_weight(h), h->xb, B, n, true, nullptr, h->amax_val, h->amax_idx, want_lp ? h->amax_sum : nullptr);
    HIP_OK(h, launch_skinny(ha, SK_BIAS_F32, s));
    // 2. accept
    *(volatile int32_t*)h->acc_host = -1;
    DraftAcceptArgs da{};
    da.val = h->amax_val; da.idx = h->amax_idx; da.ntiles = ntiles; da.B = B; da.n = n; da.ids = h->g_ids; da.ld = ld;
    da.tok = h->acc_tok; da.ticket = h->acc_ticket; da.sep_cnt = h->sep_cnt; da.sep_id = h->c.sep_token_id; da.host = h->acc_host;
    if (want_lp) { da.sum = h->amax_sum; da.lp_tok = h->acc_lp; da.lp_out = h->g_lp; da.ld_lp = max_len; }
    HIP_OK(h, launch_draft_accept(da, s));
    HIP_OK(h, hipEventRecord(h->acc_ev, s));
    HIP_OK(h, hipEventSynchronize(h->acc_ev));
    const int a = ((volatile int32_t*)h->acc_host)[0];
    const bool fired = ((volatile int32_t*)h->acc_host)[1] != 0;
    if (a < 0 || a > n) return fail(h, GITCAP_ERR_HIP, "student draft: the accept kernel published no count");
    // 3. tail: the token steps the pass did not cover
    const int t0 = a < n ? a + 1 : n;
    const bool tail = t0 < max_len && !(stop == GITCAP_STOP_ALL_SEP && fired);
    for (int t = t0; tail && t < max_len; ++t) {
        if (g_use_graph) HIP_OK(h, hipGraphLaunch((*steps)[t - 1], s));
        else if ((rc = token_step(h, B, t, max_len, want_lp, s))) return rc;
    }
    HIP_OK(h, launch_finish_steps(h->sep_cnt, B, max_len, stop, h->g_steps, s));
    if ((rc = copy_out(h, B, max_len, ids_out, steps_out, lp, s))) return rc;
    if (accepted_out) *accepted_out = a;
    ++h->draft_calls; h->draft_offered += n; h->draft_accepted += a; h->draft_tail_steps += tail ? max_len - t0 : 0;
    return 0;
}

// search: the call took search options (gitcap_student_attach_search) -- the hypothesis store joins the workspace at the first such
// call, each buffer on its own (a call repeated after a failed allocation keeps what the first one got)
int beam_workspace(gitcap_student* h, bool search = false) {
    gitcap_student::BeamWs& w = h->bw;
    const size_t R = h->R, ld = (size_t)h->Tmax + 1;
    int rc = 0;
    if (!w.memrep) {
        const int D = h->D, V = h->V;
        rc = rc ? rc : dev_alloc(h, &w.memrep, R * h->F * D);
        rc = rc ? rc : dev_alloc(h, &w.scores, R);
        rc = rc ? rc : dev_alloc(h, &w.cand_scores, R);
        rc = rc ? rc : dev_alloc(h, &w.cand_idx, R);
        rc = rc ? rc : dev_alloc(h, &w.src_rows, R);
        rc = rc ? rc : dev_alloc(h, &w.ids0, R * ld);
        rc = rc ? rc : dev_alloc(h, &w.ids1, R * ld);
        rc = rc ? rc : dev_alloc(h, &w.logits, R * (size_t)V);
        rc = rc ? rc : dev_alloc(h, &w.kvs2, (size_t)h->L * h->R * h->Tmax * 3 * D);
        rc = rc ? rc : dev_alloc(h, &w.topk_scratch, beam_topk_scratch_bytes(h->R, 1, V, 16));     // rows x chunks, whatever the split into clips x beams
        if (rc) w = gitcap_student::BeamWs{};
    }
    if (rc || !search) return rc;
    if (!w.words && (rc = dev_alloc(h, &w.words, R))) { w.words = nullptr; return rc; }
    if (!w.done && (rc = dev_alloc(h, &w.done, R))) { w.done = nullptr; return rc; }
    if (!w.hyp_len && (rc = dev_alloc(h, &w.hyp_len, R))) { w.hyp_len = nullptr; return rc; }
    if (!w.hyp_score && (rc = dev_alloc(h, &w.hyp_score, R))) { w.hyp_score = nullptr; return rc; }
    if (!w.hyp_ids && (rc = dev_alloc(h, &w.hyp_ids, R * h->Tmax))) { w.hyp_ids = nullptr; return rc; }
    if (!w.cand16_scores && (rc = dev_alloc(h, &w.cand16_scores, R * 16))) { w.cand16_scores = nullptr; return rc; }
    if (!w.cand16_idx && (rc = dev_alloc(h, &w.cand16_idx, R * 16))) { w.cand16_idx = nullptr; return rc; }
    return 0;
}

// the token loop of beam_search against the memory K|V of B * k rows in h->memkv (set_memory of the repeated rows, or the window's gather)
// co.on: every step first builds the mask of the B * k rows from the buffer that holds their current prefixes (positions 0 .. t), and
// the ranking runs its BAN form: banned columns are -inf ahead of the log-softmax
// pr.ids set (max_len counts the prompt): the rows start from the staged prompts, clip b's row for its k beams, and while a clip is
// inside its prompt the bookkeeping step appends the prompt's token to every one of its rows instead of ranking (the FORCED form)
// se.on (gitcap_student_attach_search): the bookkeeping is the teacher's (search.hip: launch_beam_init / _step / _finish over this
// workspace), step t being its cur_len = t + 1.  Those kernels take id rows whose pitch is the call's max_len, so the two id buffers
// are used at that pitch (they hold Tmax + 1 columns per row) and every launch that reads them is told so.  K = k * se.pn candidates
// are ranked under se.rp; ids_out is [B][se.n][max_len].  A done clip's k rows are padded by the step kernel -- SEP appended to a
// copy of row 0's prefix, src_rows = 0, so the K/V rows the gather gives them are row 0's as well: ids and cache stay consistent,
// the PAD-key mask (by id) sees row 0's ids.  Whatever those rows compute is read by nobody else: a row attends to its own cache and
// its clip's memory only, its logits rank among its own clip's candidates only, and the step kernel reads no candidate of a done
// clip and leaves its hypotheses frozen.  No host decision: all max_len - 1 steps run.
int beam_loop(gitcap_student* h, int B, int k, int max_len, int64_t* ids_out, hipStream_t s, const ConsOpt& co, const PromptArgs& pr,
              const StudentSearch& se) {
    const int rows = B * k, D = h->D, V = h->V, ld = se.on ? max_len : h->Tmax + 1, K = se.on ? k * se.pn : k;
    int rc = 0;
    gitcap_student::BeamWs& w = h->bw;
    const BeamBuffers bb{w.ids0, w.ids1, w.words, w.hyp_ids, w.scores, w.hyp_score, w.src_rows, w.done, w.hyp_len};
    const PromptArgs tab = table_prompt(h, pr, max_len - 1);        // (at least one free position)
    if (pr.ids) {
        if ((rc = write_prompt_tables(h, pr, B, s))) return rc;
        const StudentPromptStageArgs sa{h->prm_ids, h->Tmax + 1, h->prm_len, rows, k, max_len - 1, h->c.cls_token_id, w.ids0, ld, nullptr, 0, 1};
        HIP_OK(h, launch_student_prompt_stage(sa, s));
    } else {
        HIP_OK(h, launch_fill_i64(w.ids0, ld, rows, h->c.cls_token_id, s));
    }
    if (se.on) {            // scores [0, -1e9, ..], src_rows the identity, no clip done, no hypothesis stored (column 0 is CLS already)
        HIP_OK(h, launch_beam_init(bb, B, k, se.n, max_len, h->c.cls_token_id, s));
    } else {
        hipLaunchKernelGGL(beam_scores_init_kernel, dim3((rows + 63) / 64), dim3(64), 0, s, w.scores, rows, k);
        HIP_OK(h, hipGetLastError());
    }
    int64_t *cur = w.ids0, *nxt = w.ids1;
    bf16_t* const kvs_home = h->kvs;
    const size_t kv_layer = (size_t)h->R * h->Tmax * 3 * D;
    TextReq q;                  // one position of every beam row -> its logits
    q.ld_ids = ld; q.rows = rows; q.T = 1; q.logits_out = w.logits;
    CandArgs ca{};              // the K best of every clip's k * V candidates (without search options: K = k, no penalty)
    ca.logits = w.logits; ca.ld = V; ca.beam_scores = w.scores; ca.ld_ids = ld; ca.rp = se.on ? se.rp : 1.0f; ca.B = B; ca.beams = k; ca.V = V;
    ca.out_scores = se.on ? w.cand16_scores : w.cand_scores; ca.out_idx = se.on ? w.cand16_idx : w.cand_idx;
    const HeadBan bn{h->ban_mask, h->ban_ld};
    if (co.on) ca.bn = &bn;
    BeamStepArgs bs{};
    bs.n = se.n; bs.cand_scores = ca.out_scores; bs.cand_idx = ca.out_idx; bs.B = B; bs.beams = k; bs.K = K; bs.V = V; bs.max_len = max_len;
    bs.eos = h->c.sep_token_id; bs.length_penalty = se.length_penalty; bs.sampled = false; bs.prompt = pr.ids ? &tab : nullptr;
    for (int t = 0; t + 1 < max_len && !rc; ++t) {                      // the token at position t is decoded, position t + 1 chosen
        if (t > 0) {                                                    // rows continue beam src_rows[r]: positions 0 .. t-1, all layers
            bf16_t* other = h->kvs == kvs_home ? w.kvs2 : kvs_home;
            const hipError_t eg = launch_gather_txt_rows(h->kvs, other, w.src_rows, rows, t, h->Tmax, 3 * D, h->L, kv_layer, s);
            if (eg != hipSuccess) { rc = fail(h, GITCAP_ERR_HIP, std::string("student_beam_search: gather_txt_rows: ") + hipGetErrorString(eg)); break; }   // (h->kvs is restored below on every path)
            h->kvs = other;
        }
        q.ids = cur; q.t0 = t;
        rc = text_forward(h, q, s);
        if (rc) break;
        if (co.on) {
            const hipError_t eb = launch_ban_mask(cur, ld, rows, t + 1, co.ngram, co.min_length, h->c.sep_token_id, co.suppress, co.n_suppress, V,
                                                  h->ban_mask, h->ban_ld, s);
            if (eb != hipSuccess) { rc = fail(h, GITCAP_ERR_HIP, std::string("student_beam_search: ban_mask: ") + hipGetErrorString(eb)); break; }
        }
        ca.prefix_ids = cur; ca.cur_len = t + 1;                        // (read under a penalty only)
        hipError_t e = launch_beam_topk(ca, K, w.topk_scratch, s);
        if (e != hipSuccess) { rc = fail(h, GITCAP_ERR_HIP, std::string("student_beam_search: beam_topk: ") + hipGetErrorString(e)); break; }
        if (se.on) {
            bs.cur_len = t + 1; bs.cur = cur == w.ids0 ? 0 : 1;
            if (launch_beam_step(bb, bs, s) != hipSuccess) { rc = fail(h, GITCAP_ERR_HIP, "student_beam_search: beam step launch"); break; }
        } else {
            const StudentBeamStepArgs st{w.cand_scores, w.cand_idx, cur, nxt, w.scores, w.src_rows, B, k, V, t, ld, pr.ids ? &tab : nullptr};
            if (launch_student_beam_step(st, s) != hipSuccess) { rc = fail(h, GITCAP_ERR_HIP, "student_beam_search: beam step launch"); break; }
        }
        std::swap(cur, nxt);
    }
    h->kvs = kvs_home;                                                  // (the captured greedy graphs hold this pointer)
    if (rc) return rc;
    if (se.on) {            // the n hypotheses of every clip by rank -> the caller's buffers
        HIP_OK(h, launch_beam_finish(bb, se.n, B, max_len, h->c.sep_token_id, BeamFinishOut{ids_out, se.scores, nullptr, nullptr}, s));
        if (se.lengths) {
            hipLaunchKernelGGL(student_hyp_lengths_kernel, dim3((B * se.n + 63) / 64), dim3(64), 0, s, w.hyp_score, w.hyp_len, se.n, B * se.n, se.lengths);
            HIP_OK(h, hipGetLastError());
        }
        return 0;
    }
    hipLaunchKernelGGL(student_beam_finish_kernel, dim3(B), dim3(64), 0, s, cur, ids_out, k, ld, max_len);
    HIP_OK(h, hipGetLastError());
    return 0;
}

// ---- memory-token window -----------------------------------------------------------------------------------------------------
// A memory token is one frame's own stage-3 mean and its cross-attention K|V rows are W_kv . token + b, no positional term, from a
// GEMM whose output rows do not depend on each other: everything per frame is computed once, at the push, and a caption of the
// window only orders the F rows (student_window_gather_kernel) in front of the token loop of the full call.
// partial (gitcap_student_window_greedy_partial): a window that is not full yet gives the n < mem_tokens tokens pushed since the reset,
// oldest first, as slots 0 .. n - 1 of every row, and every row's key table entry says n: the varlen launches, a row of which is
// bit for bit the plain launch at nkeys = n.  *frames (nullable, written when the call succeeds) = the tokens the caption sees.
int window_memory(gitcap_student* h, const char* who, int k, hipStream_t s, bool partial = false, int* frames = nullptr) {
    if (!h->win_ring || (partial ? h->win.count < 1 : !h->win.full()))
        return fail(h, GITCAP_ERR_STATE, std::string(who) + (partial ? ": no token pushed since the reset" : ": fewer than mem_tokens tokens pushed since the reset"));
    const int rows = h->win_B * k, D = h->D, F = h->F, n = h->win.full() ? F : h->win.count;
    HIP_OK(h, h->win_order.before_read(s));
    h->have_memory = false;
    if (n < F)
        if (int rc = write_key_tables(h, rows, [&](int r) { return std::make_pair(r * F, n); }, s)) return rc;
    h->ragged = n < F;
    // the oldest token's slot: the head of a full ring, slot 0 of one that has not wrapped
    hipLaunchKernelGGL(student_window_gather_kernel, dim3(rows * n, h->L), dim3(64), 0, s, h->win_ring, h->memkv, F, (h->win.head + F - n) % F, k,
                       2 * D / 8, (size_t)h->win_B * F * 2 * D, (size_t)h->R * F * 2 * D, n);
    HIP_OK(h, hipGetLastError());
    HIP_OK(h, h->win_order.after_read(s));
    if (frames) *frames = n;
    h->cur_B = rows;
    h->have_memory = true;
    return 0;
}

// The greedy entry points.  who = the entry point's name in every message; parts / refuse = the attachments it takes -- before the
// checks: a refused call has consumed them -- and refuses (take); draft set: the loop verifies it.  source(opts, stream, &B) does the
// checks of the entry point's own arguments and state and provides the memory K|V of its B rows: from the caller's `memory`
// (memory_source; set_memory reads the caller's buffer: outside the graphs), the window's ring or the pool's.  early_bad: a fault in
// the source's arguments that is reported as the family's first "bad arguments".
template <typename Source>
int greedy_entry(gitcap_student* h, const char* who, unsigned parts, unsigned refuse, const Draft* draft, int max_len, int stop, int64_t* ids_out,
                 int32_t* steps_out, void* stream, Source source, bool early_bad = false) {
    const std::string w(who);
    if (!h) return fail(h, GITCAP_ERR_ARG, w + ": null handle");
    StudentOpts o;
    if (int bad = take(h, w, parts, refuse | OPT_SO, &o)) return bad;         // (search options are the beam family's)
    if (early_bad || !ids_out || max_len <= 0) return fail(h, GITCAP_ERR_ARG, w + ": bad arguments");
    if (max_len + 1 > h->Tmax) return fail(h, GITCAP_ERR_ARG, w + ": max_len exceeds max_text_len");
    if (stop != GITCAP_STOP_NEVER && stop != GITCAP_STOP_ALL_SEP) return fail(h, GITCAP_ERR_ARG, w + ": unknown stop rule");
    if (int bad = lp_check(h, who, o.lp, max_len)) return bad;
    if (int bad = tk_check(h, who, o.tk, max_len)) return bad;
    if (int bad = cons_check(h, w, o.co, max_len, 1)) return bad;
    if (o.pr.ids && o.pr.max_len > max_len) return fail(h, GITCAP_ERR_ARG, w + ": the attached prompt is longer than max_len");
    if (draft && !draft->ids) return fail(h, GITCAP_ERR_ARG, w + ": null draft_ids");
    if (draft && (draft->n < 1 || draft->n > max_len || draft->ld < draft->n + 1))
        return fail(h, GITCAP_ERR_ARG, w + ": n_draft outside [1, max_len], or ld_draft < n_draft + 1");
    GUARD(h);
    hipStream_t s = (hipStream_t)stream;
    int B = 0;
    if (int rc = source(o, w, s, &B)) return rc;
    if (draft) return greedy_draft_core(h, B, draft->ids, draft->ld, draft->n, max_len, stop, ids_out, steps_out, draft->accepted_out, s, o.lp);
    return greedy_loop(h, B, max_len, stop, ids_out, steps_out, s, o.lp, o.tk, o.co, o.pr);
}
constexpr unsigned GREEDY_PARTS = OPT_LP | OPT_TK | OPT_CO | OPT_PR, DRAFT_REFUSES = OPT_PR | OPT_CO | OPT_TK;
// the caller's memory of B clips, following the counts the call took
auto memory_source(gitcap_student* h, const float* memory, int B) {
    return [=](const StudentOpts& o, const std::string& who, hipStream_t s, int* rows) -> int {
        const Counts* ragged = nullptr;
        if (int bad = counts_for_call(h, who, o.fc, B, &ragged)) return bad;
        *rows = B;
        return set_memory(h, memory, B, s, ragged);
    };
}
// the window's win_B clips; partial: the window need not be full (window_memory), *frames_out (host, nullable) = the tokens the caption saw
auto window_source(gitcap_student* h, bool partial = false, int32_t* frames_out = nullptr) {
    return [=](const StudentOpts&, const std::string& who, hipStream_t s, int* rows) -> int {
        if (!h->finalized) return fail(h, GITCAP_ERR_STATE, who + ": weights not finalized");
        *rows = h->win_B;
        return window_memory(h, who.c_str(), 1, s, partial, frames_out);
    };
}

// The two beam entry points, in greedy_entry's shape.  early(&B): the source's checks that come ahead of the family's, and its clips;
// source(opts, stream): its other checks, then beam_workspace and the memory K|V of the B * k rows.
template <typename Early, typename Source>
int beam_entry(gitcap_student* h, const char* who, unsigned parts, unsigned refuse, int k, int max_len, int64_t* ids_out, void* stream, Early early,
               Source source) {
    const std::string w(who);
    if (!h) return fail(h, GITCAP_ERR_ARG, w + ": null handle");
    StudentOpts o;
    int B = 0, bad = take(h, w, parts, refuse, &o);
    if (bad || (bad = early(&B))) return bad;
    if (!ids_out || B <= 0 || k <= 0 || max_len < 2) return fail(h, GITCAP_ERR_ARG, w + ": bad arguments");
    if (k > 16) return fail(h, GITCAP_ERR_ARG, w + ": at most 16 beams");
    if ((int64_t)B * k > h->R) return fail(h, GITCAP_ERR_ARG, w + ": B * k exceeds max_rows");
    if (max_len > h->Tmax) return fail(h, GITCAP_ERR_ARG, w + ": max_len exceeds max_text_len + 1");
    StudentSearch& se = o.se;
    if (se.on) {
        if (se.pn == 0) se.pn = k;
        if (se.n > k) return fail(h, GITCAP_ERR_ARG, w + ": the attached num_keep_best exceeds k");
        if (se.pn > k || k * se.pn > 16) return fail(h, GITCAP_ERR_ARG, w + ": the attached per_node_beam_size exceeds k, or k * per_node_beam_size > 16 candidates");
        // with one candidate per beam a SEP candidate leaves a clip short of k live beams, which the reference asserts against
        // (model.py:606); the device bookkeeping has no way to report it, so refuse up front
        if (se.pn < 2) return fail(h, GITCAP_ERR_ARG, w + ": the attached search needs per_node_beam_size >= 2, so k >= 2 (model.py:606)");
    }
    if ((bad = cons_check(h, w, o.co, max_len, se.on ? k * se.pn : k))) return bad;
    if (o.pr.ids && o.pr.max_len > max_len - 1) return fail(h, GITCAP_ERR_ARG, w + ": the attached prompt is longer than max_len - 1");
    GUARD(h);
    hipStream_t s = (hipStream_t)stream;
    if (int rc = source(o, s)) return rc;
    return beam_loop(h, B, k, max_len, ids_out, s, o.co, o.pr, se);
}

// ---- stream pool ---------------------------------------------------------------------------------------------------------------
// The memory K|V of a pool call: decoder row r = stream ids[r] (non-null: greedy_entry's early_bad; in range, distinct, not empty), its
// last n_r = min(count, F) tokens oldest first, rows packed as set_memory packs clips of different length -- the layout and the key
// tables of gitcap_student_attach_frame_counts, so the token loop is that call's.  Every n_r == F: the packed layout is the dense
// one and the loop takes the dense launches, as a full lockstep window's.  frames (host, nullable) = n_r.
// (The teacher's pool_plan checks a row's id, duplicate and emptiness in one pass: the two report different faults first.)
// k > 1 (gitcap_student_pool_beam_search): decoder rows r * k .. r * k + k - 1 are the beams of stream ids[r].  The gather is the same
// launch -- every stream's rows are copied once -- and the k rows read them through the key tables, as set_memory(.., ragged, k) has
// them: nothing is repeated, so the tables are written whether or not every stream is full.
int pool_memory(gitcap_student* h, const std::string& w, const int32_t* ids, int B, hipStream_t s, int32_t* frames, int k = 1) {
    if (B < 1 || B > h->R) return fail(h, GITCAP_ERR_ARG, w + ": B outside [1, max_rows]");
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, w + ": weights not finalized");
    if (!h->pool_ring) return fail(h, GITCAP_ERR_STATE, w + ": no pool (gitcap_student_pool_reset first)");
    for (int r = 0; r < B; ++r) {
        if (ids[r] < 0 || ids[r] >= h->pool_S)
            return fail(h, GITCAP_ERR_ARG, w + ": row " + std::to_string(r) + " names stream " + std::to_string(ids[r]) + ", outside [0, " +
                        std::to_string(h->pool_S) + ")");
        for (int q = 0; q < r; ++q)
            if (ids[q] == ids[r]) return fail(h, GITCAP_ERR_ARG, w + ": stream " + std::to_string(ids[r]) + " is named twice");
    }
    for (int r = 0; r < B; ++r)
        if (h->pool[(size_t)ids[r]].count < 1) return fail(h, GITCAP_ERR_STATE, w + ": stream " + std::to_string(ids[r]) + " holds no token");
    const int D = h->D, F = h->F;
    int32_t* const tab = h->pool_tab_host.p;
    HIP_OK(h, h->pool_tab_host.wait());
    bool dense = true;
    int off = 0;
    for (int r = 0; r < B; ++r) {
        const RingCursor& c = h->pool[(size_t)ids[r]];
        int32_t* t = tab + 4 * r;
        t[0] = ids[r] * F; t[1] = c.oldest(); t[2] = c.count; t[3] = off;
        off += c.count;
        dense = dense && c.count == F;
    }
    HIP_OK(h, h->pool_order.before_read(s));
    h->have_memory = false;
    HIP_OK(h, h->pool_tab_host.copy(h->pool_tab, 0, (size_t)B * 4, s));
    HIP_OK(h, h->pool_tab_host.mark(s));
    const bool ragged = !dense || k > 1;
    if (ragged)
        if (int rc = write_key_tables(h, B * k, [&](int r) { return std::make_pair((int)tab[4 * (r / k) + 3], (int)tab[4 * (r / k) + 2]); }, s)) return rc;
    h->ragged = ragged;
    hipLaunchKernelGGL(student_pool_gather_kernel, dim3(B * F, h->L), dim3(64), 0, s, h->pool_ring, h->memkv, h->pool_tab, F, 2 * D / 8,
                       (size_t)h->pool_S * F * 2 * D, (size_t)h->R * F * 2 * D);
    HIP_OK(h, hipGetLastError());
    HIP_OK(h, h->pool_order.after_read(s));
    if (frames)
        for (int r = 0; r < B; ++r) frames[r] = tab[4 * r + 2];
    h->cur_B = B * k;
    h->have_memory = true;
    return 0;
}

}  // namespace

extern "C" {

int gitcap_student_greedy(gitcap_student_t* h, const float* memory, int B, int max_len, int stop, int64_t* ids_out,
                          int32_t* steps_out, void* stream) {
    return greedy_entry(h, "student_greedy", GREEDY_PARTS | OPT_FC, 0, nullptr, max_len, stop, ids_out, steps_out, stream, memory_source(h, memory, B));
}

// StudentCandidateV1.beam_search (model.py:189-318) on the device with the exact KV cache: k beams per clip as rows
// b * k + i, no end-of-sequence handling (as the reference), no host round trip.  The reference lets every beam propose its
// top k and keeps the k best of the k * k candidates; the k best of ALL beams x vocabulary candidates are the same set (a
// candidate among the global k best is among its own beam's k best), which is what beam_topk ranks (log_softmax + beam
// score, best first, ties to the smaller beam-major index).  Before the first step only beam 0 is live (score 0, the others
// -1e9), so the k rows start as the top k of the single prefix [CLS] (model.py:221-227).  After every step the self-attention
// K/V rows follow their beams (gather into the second cache buffer) and so do the id rows the PAD-key mask reads.
int gitcap_student_beam_search(gitcap_student_t* h, const float* memory, int B, int k, int max_len, int64_t* ids_out, void* stream) {
    const char* who = "student_beam_search";
    return beam_entry(h, who, OPT_FC | OPT_CO | OPT_PR | OPT_SO, 0, k, max_len, ids_out, stream,
        [&](int* clips) { *clips = B; return memory ? 0 : fail(h, GITCAP_ERR_ARG, "student_beam_search: bad arguments"); },
        [&](const StudentOpts& o, hipStream_t s) -> int {
            const Counts* ragged = nullptr;
            if (int bad = counts_for_call(h, who, o.fc, B, &ragged)) return bad;
            if (int rc = beam_workspace(h, o.se.on)) return rc;
            if (ragged) return set_memory(h, memory, B, s, ragged, k);      // the k beams of a clip read its packed K|V rows through the tables: nothing is repeated
            hipLaunchKernelGGL(repeat_rows_kernel, dim3(4, B * k), dim3(256), 0, s, memory, h->bw.memrep, k, h->F * h->D / 4);
            HIP_OK(h, hipGetLastError());
            return set_memory(h, h->bw.memrep, B * k, s);
        });
}

int gitcap_student_window_reset(gitcap_student_t* h, int B) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "student_window_reset: null handle");
    if (int bad = take(h, "student_window_reset", 0, OPT_FC)) return bad;
    if (B < 0 || B > h->R) return fail(h, GITCAP_ERR_ARG, "student_window_reset: B outside 0..max_rows");
    GUARD(h);
    if (h->win_ring && B != h->win_B) {
        HIP_OK(h, hipDeviceSynchronize());          // pushes or window calls in flight may still use the ring
        (void)hipFree(h->win_ring); (void)hipFree(h->win_stage);
        h->win_ring = h->win_stage = nullptr;
    }
    h->win_B = 0;
    h->win.reset(h->F);
    if (B == 0) return 0;
    HIP_OK(h, h->win_order.ensure());
    if (!h->win_ring) {
        const size_t rows = (size_t)B * h->F;
        hipError_t e = hipMalloc((void**)&h->win_ring, (size_t)h->L * rows * 2 * h->D * sizeof(bf16_t));
        if (e == hipSuccess && (e = hipMalloc((void**)&h->win_stage, rows * h->D * sizeof(bf16_t))) != hipSuccess) {
            (void)hipFree(h->win_ring);
            h->win_ring = nullptr;
        }
        if (e != hipSuccess) {
            h->win_ring = h->win_stage = nullptr;
            return fail(h, GITCAP_ERR_NOMEM, std::string("hipMalloc memory-token window: ") + hipGetErrorString(e));
        }
    }
    h->win_B = B;
    return 0;
}

int gitcap_student_window_push(gitcap_student_t* h, const float* memory, int B, int n, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "student_window_push: null handle");
    if (int bad = take(h, "student_window_push", 0, OPT_FC)) return bad;
    if (!memory) return fail(h, GITCAP_ERR_ARG, "student_window_push: null memory");
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "student_window_push: weights not finalized");
    if (!h->win_ring) return fail(h, GITCAP_ERR_STATE, "student_window_push: no window (gitcap_student_window_reset first)");
    if (B != h->win_B || n < 1 || n > h->F) return fail(h, GITCAP_ERR_ARG, "student_window_push: B differs from the reset's, or n outside [1, mem_tokens]");
    GUARD(h);
    hipStream_t s = (hipStream_t)stream;
    HIP_OK(h, h->win_order.before_push(s));
    const int D = h->D, F = h->F, n1 = h->win.first_run(n), n2 = n - n1;
    const int64_t total = (int64_t)B * n * (D / 4);
    hipLaunchKernelGGL(student_window_stage_kernel, dim3((unsigned)std::min<int64_t>((total + 255) / 256, 1024)), dim3(256), 0, s, memory,
                       h->win_stage, B, n, n1, D / 4);
    HIP_OK(h, hipGetLastError());
    const size_t ring_layer = (size_t)B * F * 2 * D;
    for (int l = 0; l < h->L; ++l) {
        const StuLayer& Ly = h->layers[l];
        // k | v of the new tokens: set_memory's GEMM (same launch form whatever M), its output rows the ring slots head .. head + n1 - 1
        // of every clip and, wrapped, 0 .. n2 - 1
        bf16_t* ring = h->win_ring + (size_t)l * ring_layer;
        int rc = sk_full(h, s, SK_BIAS_BF16, h->win_stage, D, Ly.ca_in_w + (size_t)D * D, Ly.ca_in_b + D, B * n1, 2 * D, D, ring, 2 * D,
                         n1, F, h->win.head);
        if (!rc && n2)
            rc = sk_full(h, s, SK_BIAS_BF16, h->win_stage + (size_t)B * n1 * D, D, Ly.ca_in_w + (size_t)D * D, Ly.ca_in_b + D, B * n2, 2 * D, D,
                         ring, 2 * D, n2, F, 0);
        if (rc) { h->win.clear(); return rc; }        // some slots may be half written: the window is emptied
    }
    HIP_OK(h, h->win_order.after_push(s));
    h->win.push(n);
    return 0;
}

int gitcap_student_window_greedy(gitcap_student_t* h, int max_len, int stop, int64_t* ids_out, int32_t* steps_out, void* stream) {
    return greedy_entry(h, "student_window_greedy", GREEDY_PARTS, OPT_FC, nullptr, max_len, stop, ids_out, steps_out, stream, window_source(h));
}

int gitcap_student_window_greedy_partial(gitcap_student_t* h, int max_len, int stop, int64_t* ids_out, int32_t* steps_out, int32_t* frames_out,
                                         void* stream) {
    return greedy_entry(h, "student_window_greedy_partial", GREEDY_PARTS, OPT_FC, nullptr, max_len, stop, ids_out, steps_out, stream,
                        window_source(h, true, frames_out));
}

int gitcap_student_greedy_draft(gitcap_student_t* h, const float* memory, int B, const int64_t* draft_ids, int ld_draft, int n_draft,
                                int max_len, int stop, int64_t* ids_out, int32_t* steps_out, int32_t* accepted_out, void* stream) {
    const Draft d{draft_ids, ld_draft, n_draft, accepted_out};
    return greedy_entry(h, "student_greedy_draft", OPT_LP | OPT_FC, DRAFT_REFUSES, &d, max_len, stop, ids_out, steps_out, stream, memory_source(h, memory, B));
}

int gitcap_student_window_greedy_draft(gitcap_student_t* h, const int64_t* draft_ids, int ld_draft, int n_draft, int max_len, int stop,
                                       int64_t* ids_out, int32_t* steps_out, int32_t* accepted_out, void* stream) {
    const Draft d{draft_ids, ld_draft, n_draft, accepted_out};
    return greedy_entry(h, "student_window_greedy_draft", OPT_LP, OPT_FC | DRAFT_REFUSES, &d, max_len, stop, ids_out, steps_out, stream, window_source(h));
}

int gitcap_student_attach_token_logprobs(gitcap_student_t* h, float* logprobs_out, int ld) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "student_attach_token_logprobs: null handle");
    if (!logprobs_out) { h->pending.lp = LpAttach{}; return 0; }
    if (ld < 1 || ((uintptr_t)logprobs_out & 3) != 0) return fail(h, GITCAP_ERR_ARG, "student_attach_token_logprobs: ld < 1 or a misaligned pointer");
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "student_attach_token_logprobs: weights not finalized");
    GUARD(h);
    if (!h->g_lp) {                             // first attach: sized as amax_val (covers the verify pass's B * n rows)
        const size_t Mt = (size_t)h->Mt, ntiles = ((size_t)h->V + 15) / 16;
        int rc;
        if ((rc = h->amax_sum ? 0 : dev_alloc(h, &h->amax_sum, Mt * ntiles)) || (rc = dev_alloc(h, &h->acc_lp, Mt)) || (rc = dev_alloc(h, &h->g_lp, Mt))) {
            h->g_lp = nullptr;
            return rc;
        }
    }
    h->pending.lp = LpAttach{logprobs_out, ld};
    return 0;
}

int gitcap_student_attach_top_logprobs(gitcap_student_t* h, int k, int64_t* top_ids, float* top_lp, int ld) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "student_attach_top_logprobs: null handle");
    if (k == 0 || !top_ids || !top_lp) { h->pending.tk = TopkAttach{}; return 0; }
    if (const char* bad = tk_attach_bad(k, top_ids, top_lp, ld)) return fail(h, GITCAP_ERR_ARG, std::string("student_attach_top_logprobs: ") + bad);
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "student_attach_top_logprobs: weights not finalized");
    if (!head_topk_ok(h->D, false)) return fail(h, GITCAP_ERR_ARG, "student_attach_top_logprobs: no top-k kernel for this decoder width");
    GUARD(h);
    {   // first attach: the sum partial (sized as amax_val) and the loops' own rows at the largest k; each buffer on its own, so
        // that an attach repeated after a failed allocation keeps what the first one got
        const size_t Mt = (size_t)h->Mt, ntiles = ((size_t)h->V + 15) / 16;
        int rc;
        if (!h->amax_sum && (rc = dev_alloc(h, &h->amax_sum, Mt * ntiles))) { h->amax_sum = nullptr; return rc; }
        if (!h->g_tk_ids && (rc = dev_alloc(h, &h->g_tk_ids, Mt * HEAD_TOPK_MAX))) { h->g_tk_ids = nullptr; return rc; }
        if (!h->g_tk_lp && (rc = dev_alloc(h, &h->g_tk_lp, Mt * HEAD_TOPK_MAX))) { h->g_tk_lp = nullptr; return rc; }
    }
    h->pending.tk = TopkAttach{k, top_ids, top_lp, ld};
    return 0;
}

int gitcap_student_attach_constraints(gitcap_student_t* h, const gitcap_constraints* c) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "student_attach_constraints: null handle");
    h->pending.co = ConsOpt{};
    if (!c) return 0;                                        // detach
    if (c->no_repeat_ngram_size < 0 || c->min_length < 0 || c->n_suppress < 0) return fail(h, GITCAP_ERR_ARG, "student_attach_constraints: a negative field");
    if (c->n_suppress > BAN_REC_MAX_SUPPRESS) return fail(h, GITCAP_ERR_ARG, "student_attach_constraints: n_suppress > 256");
    if (c->n_suppress > 0 && (!c->suppress || ((uintptr_t)c->suppress & 3) != 0))
        return fail(h, GITCAP_ERR_ARG, "student_attach_constraints: n_suppress > 0 with a null or misaligned suppress pointer");
    if (h->V > 131072) return fail(h, GITCAP_ERR_ARG, "student_attach_constraints: the ban mask takes a vocabulary of at most 131072 columns");
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "student_attach_constraints: weights not finalized");
    GUARD(h);
    {   // first attach: the mask of the step's rows (ld even, >= ceil(V / 16)), the record and its page-locked header; each on its
        // own, so that an attach repeated after a failed allocation keeps what the first one got
        int rc;
        h->ban_ld = (((h->V + 15) / 16) + 1) & ~1;
        if (!h->ban_mask && (rc = dev_alloc(h, &h->ban_mask, (size_t)h->R * (size_t)h->ban_ld))) { h->ban_mask = nullptr; return rc; }
        if (!h->ban_rec && (rc = dev_alloc(h, &h->ban_rec, (size_t)BAN_REC_WORDS))) { h->ban_rec = nullptr; return rc; }
        HIP_OK(h, h->ban_host.ensure(BAN_REC_HEADER));
    }
    h->pending.co = ConsOpt{true, c->no_repeat_ngram_size, c->min_length, c->n_suppress ? c->suppress : nullptr, c->n_suppress};
    return 0;
}

int gitcap_student_attach_prompt(gitcap_student_t* h, const int64_t* prompt_ids, int ld, const int32_t* lengths, int min_len, int max_len) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "student_attach_prompt: null handle");
    h->pending.pr = PromptArgs{};
    if (!prompt_ids && !lengths) return 0;                   // detach
    if (!prompt_ids || !lengths) return fail(h, GITCAP_ERR_ARG, "student_attach_prompt: prompt_ids and lengths are both required");
    if (((uintptr_t)prompt_ids & 7) != 0 || ((uintptr_t)lengths & 3) != 0) return fail(h, GITCAP_ERR_ARG, "student_attach_prompt: a misaligned pointer");
    if (min_len < 1 || max_len < min_len || ld < max_len) return fail(h, GITCAP_ERR_ARG, "student_attach_prompt: need 1 <= min_len <= max_len <= ld");
    if (max_len > h->Tmax) return fail(h, GITCAP_ERR_ARG, "student_attach_prompt: max_len exceeds max_text_len + 1");
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "student_attach_prompt: weights not finalized");
    GUARD(h);
    {   // first attach: the handle's own tables, each on its own (an attach repeated after a failed allocation keeps what the first got)
        int rc;
        if (!h->prm_ids && (rc = dev_alloc(h, &h->prm_ids, (size_t)h->R * ((size_t)h->Tmax + 1)))) { h->prm_ids = nullptr; return rc; }
        if (!h->prm_len && (rc = dev_alloc(h, &h->prm_len, (size_t)h->R))) { h->prm_len = nullptr; return rc; }
    }
    h->pending.pr = PromptArgs{prompt_ids, ld, lengths, min_len, max_len};
    return 0;
}

int gitcap_student_attach_search(gitcap_student_t* h, const gitcap_student_search_options* o) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "student_attach_search: null handle");
    h->pending.se = StudentSearch{};
    if (!o) return 0;                                        // detach
    if (o->num_keep_best < 1 || o->num_keep_best > 16 || o->per_node_beam_size < 0 || o->per_node_beam_size == 1 || o->per_node_beam_size > 16)
        return fail(h, GITCAP_ERR_ARG, "student_attach_search: num_keep_best outside [1, 16], or per_node_beam_size not 0 or in [2, 16]");
    if (!std::isfinite(o->length_penalty) || !(o->repetition_penalty > 0.f) || !std::isfinite(o->repetition_penalty))
        return fail(h, GITCAP_ERR_ARG, "student_attach_search: length_penalty must be finite, repetition_penalty > 0 and finite");
    if (!o->scores_out || (((uintptr_t)o->scores_out | (uintptr_t)o->lengths_out) & 3) != 0)
        return fail(h, GITCAP_ERR_ARG, "student_attach_search: null scores_out or a misaligned pointer");
    h->pending.se = StudentSearch{true, o->num_keep_best, o->length_penalty, o->per_node_beam_size, o->repetition_penalty, o->scores_out, o->lengths_out};
    return 0;
}

int gitcap_student_score(gitcap_student_t* h, const int64_t* ids, int ld_ids, int rows, int T, const int32_t* lengths, int64_t ignore_id,
                         float* token_lp, int ld_lp, float* row_sum, int32_t* row_cnt, int64_t* top1_ids, float* top1_lp, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "student_score: null handle");
    StudentOpts o;
    if (int bad = take(h, "student_score", OPT_TK, OPT_SO, &o)) return bad;
    const TopkAttach& tk = o.tk;
    if (int bad = tk_check(h, "student_score", tk, T - 1)) return bad;
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "student_score: weights not finalized");
    if (!h->have_memory) return fail(h, GITCAP_ERR_STATE, "student_score before set_memory");
    if (T < 2 || ld_ids < T) return fail(h, GITCAP_ERR_ARG, "student_score: T < 2 (CLS and at least one token) or ld_ids < T");
    if (token_lp && ld_lp < T - 1) return fail(h, GITCAP_ERR_ARG, "student_score: ld_lp < T - 1");
    GUARD(h);
    int rc;
    if (!h->amax_sum && (rc = dev_alloc(h, &h->amax_sum, (size_t)h->Mt * (((size_t)h->V + 15) / 16)))) return rc;
    if (!h->score_buf && (rc = dev_alloc(h, &h->score_buf, 2 * (size_t)h->Mt))) return rc;
    const ScoreReq sq{lengths, ignore_id, token_lp, ld_lp, row_sum, row_cnt, top1_ids, top1_lp, tk};
    TextReq q;
    q.ids = ids; q.ld_ids = ld_ids; q.rows = rows; q.T = T; q.score = &sq;
    return text_forward(h, q, (hipStream_t)stream);
}

// The per-frame attribution of given captions: gitcap_student_score's pass without the head, its cross-attention probabilities kept
int gitcap_student_attention(gitcap_student_t* h, const int64_t* ids, int ld_ids, int rows, int T, int layer, const int32_t* lengths,
                             float* frame_mass, int ld_f, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "student_attention: null handle");
    if (int bad = take(h, "student_attention", 0, OPT_SO)) return bad;
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "student_attention: weights not finalized");
    if (!h->have_memory) return fail(h, GITCAP_ERR_STATE, "student_attention before set_memory");
    if (!frame_mass || T < 1 || ld_ids < T || ld_f < h->F || layer < -1 || layer >= h->L || (((uintptr_t)frame_mass | (uintptr_t)lengths) & 3) != 0)
        return fail(h, GITCAP_ERR_ARG, "student_attention: null or misaligned output, T < 1, ld_ids < T, ld_f < mem_tokens, or layer outside [-1, layers)");
    if (rows <= 0 || (int64_t)rows * T > h->Mt) return fail(h, GITCAP_ERR_ARG, "student_attention: rows x T beyond the handle's row workspace");
    GUARD(h);
    int rc;
    if (!h->att_probs && (rc = dev_alloc(h, &h->att_probs, (size_t)h->L * h->Mt * h->H * h->F))) return rc;
    TextReq q;
    q.ids = ids; q.ld_ids = ld_ids; q.rows = rows; q.T = T;
    h->att_on = true;
    rc = text_forward(h, q, (hipStream_t)stream);
    h->att_on = false;
    if (rc) return rc;
    HIP_OK(h, launch_cross_mean(h->att_probs, h->L, rows, T, h->H, h->F, layer, lengths, frame_mass, ld_f, (hipStream_t)stream));
    return 0;
}

int gitcap_student_dbg_score_target_logits(gitcap_student_t* h, float* out, int n, void* stream) {
    if (!h || !out || n <= 0) return fail(h, GITCAP_ERR_ARG, "student_dbg_score_target_logits: null argument");
    if (!h->score_buf || n > h->Mt) return fail(h, GITCAP_ERR_STATE, "student_dbg_score_target_logits: no gitcap_student_score call yet, or n beyond the workspace");
    GUARD(h);
    HIP_OK(h, hipMemcpyAsync(out, h->score_buf, (size_t)n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int gitcap_student_workspace_bytes(const gitcap_student_t* h, int64_t* bytes) {
    if (!h || !bytes) return fail(h, GITCAP_ERR_ARG, "student_workspace_bytes: null argument");
    *bytes = h->ws_bytes;
    return 0;
}

int gitcap_student_draft_stats(const gitcap_student_t* h, int64_t* out4) {
    if (!h || !out4) return fail(h, GITCAP_ERR_ARG, "student_draft_stats: null argument");
    out4[0] = h->draft_calls; out4[1] = h->draft_offered; out4[2] = h->draft_accepted; out4[3] = h->draft_tail_steps;
    return 0;
}

int gitcap_student_window_beam_search(gitcap_student_t* h, int k, int max_len, int64_t* ids_out, void* stream) {
    const char* who = "student_window_beam_search";
    return beam_entry(h, who, OPT_CO | OPT_PR | OPT_SO, OPT_FC, k, max_len, ids_out, stream,
        [&](int* clips) {
            *clips = h->win_B;
            if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "student_window_beam_search: weights not finalized");
            return h->win_ring ? 0 : fail(h, GITCAP_ERR_STATE, "student_window_beam_search: no window (gitcap_student_window_reset first)");
        },
        [&](const StudentOpts& o, hipStream_t s) { const int rc = beam_workspace(h, o.se.on); return rc ? rc : window_memory(h, who, k, s); });
}

// ---- stream pool ---------------------------------------------------------------------------------------------------------------
int gitcap_student_pool_reset(gitcap_student_t* h, int n_streams) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "student_pool_reset: null handle");
    if (int bad = take(h, "student_pool_reset", 0, OPT_FC)) return bad;
    if (n_streams < 0 || n_streams > 4096) return fail(h, GITCAP_ERR_ARG, "student_pool_reset: n_streams outside 0..4096");
    if (n_streams && !h->finalized) return fail(h, GITCAP_ERR_STATE, "student_pool_reset: weights not finalized");
    GUARD(h);
    if (h->pool_ring && n_streams != h->pool_S) {
        HIP_OK(h, hipDeviceSynchronize());          // pushes or pool calls in flight may still use the buffers
        pool_free(h);
    }
    if (n_streams == 0) return 0;
    if (!h->pool_ring) {
        const size_t S = (size_t)n_streams, F = (size_t)h->F, D = (size_t)h->D, L = (size_t)h->L, cap = (size_t)h->R * F;
        HIP_OK(h, h->pool_order.ensure());
        const size_t b_ring = L * S * F * 2 * D * sizeof(bf16_t), b_stage = cap * D * sizeof(bf16_t), b_kv = L * cap * 2 * D * sizeof(bf16_t),
                     b_slot = cap * sizeof(int32_t), b_tab = (size_t)h->R * 4 * sizeof(int32_t);
        hipError_t e = hipMalloc((void**)&h->pool_ring, b_ring);
        if (e == hipSuccess) e = hipMalloc((void**)&h->pool_stage, b_stage);
        if (e == hipSuccess) e = hipMalloc((void**)&h->pool_kv, b_kv);
        if (e == hipSuccess) e = hipMalloc((void**)&h->pool_slot, b_slot);
        if (e == hipSuccess) e = hipMalloc((void**)&h->pool_tab, b_tab);
        if (e == hipSuccess) e = h->pool_slot_host.ensure(cap);
        if (e == hipSuccess) e = h->pool_tab_host.ensure((size_t)h->R * 4);
        if (e != hipSuccess) {
            pool_free(h);
            return fail(h, GITCAP_ERR_NOMEM, std::string("hipMalloc stream pool: ") + hipGetErrorString(e));
        }
        h->pool_bytes = (int64_t)(b_ring + b_stage + b_kv + b_slot + b_tab);
        h->ws_bytes += h->pool_bytes;
        h->pool_S = n_streams;
        h->pool_cap = (int)cap;
        h->pool.resize(S);
    }
    for (RingCursor& c : h->pool) c.reset(h->F);
    return 0;
}

int gitcap_student_pool_push(gitcap_student_t* h, const float* memory, const int32_t* stream_ids, int n, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "student_pool_push: null handle");
    if (int bad = take(h, "student_pool_push", 0, OPT_FC)) return bad;
    if (!memory || !stream_ids) return fail(h, GITCAP_ERR_ARG, "student_pool_push: null memory or stream_ids");
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "student_pool_push: weights not finalized");
    if (!h->pool_ring) return fail(h, GITCAP_ERR_STATE, "student_pool_push: no pool (gitcap_student_pool_reset first)");
    if (n < 1 || n > h->pool_cap)
        return fail(h, GITCAP_ERR_ARG, "student_pool_push: n outside [1, max_rows * mem_tokens = " + std::to_string(h->pool_cap) + "]");
    std::vector<int32_t> slots((size_t)n);
    int bad = -1;
    if (const int why = pool_push_slots(h->pool, stream_ids, n, slots.data(), &bad))
        return fail(h, GITCAP_ERR_ARG, "student_pool_push: token " + std::to_string(bad) + (why == POOL_PUSH_BAD_ID
                    ? " names stream " + std::to_string(stream_ids[bad]) + ", outside [0, " + std::to_string(h->pool_S) + ")"
                    : " is more than mem_tokens = " + std::to_string(h->F) + " for stream " + std::to_string(stream_ids[bad]) + " in one push"));
    GUARD(h);
    hipStream_t s = (hipStream_t)stream;
    const int D = h->D;
    HIP_OK(h, h->pool_slot_host.wait());
    memcpy(h->pool_slot_host.p, slots.data(), (size_t)n * sizeof(int32_t));
    HIP_OK(h, h->pool_order.before_push(s));
    // From here on ring rows may be half written: a failure empties the streams this push names.
    auto enqueue = [&]() -> int {
        HIP_OK(h, h->pool_slot_host.copy(h->pool_slot, 0, (size_t)n, s));
        HIP_OK(h, h->pool_slot_host.mark(s));
        HIP_OK(h, launch_cast_bf16(memory, h->pool_stage, (int64_t)n * D, s));         // the bf16 rows set_memory's GEMM reads
        const size_t kv_layer = (size_t)h->pool_cap * 2 * D;
        for (int l = 0; l < h->L; ++l) {
            const StuLayer& Ly = h->layers[l];
            // k | v of the n tokens: set_memory's GEMM.  skinny_full_kernel<K32, SK_BIAS_BF16, false, false> is what launch_skinny
            // takes for this epilogue at every M (the head-sharing and row-prologue forms are for SK_BIAS_F32 and a pending
            // LayerNorm), and in it output row m is one MFMA chain over X row m alone -- an m-tile's padding rows are clamped copies
            // whose results are dropped -- so a row has the same bits at M = 1, 2, 17 or max_rows * mem_tokens.
            if (int rc = sk_full(h, s, SK_BIAS_BF16, h->pool_stage, D, Ly.ca_in_w + (size_t)D * D, Ly.ca_in_b + D, n, 2 * D, D,
                                 h->pool_kv + (size_t)l * kv_layer, 2 * D))
                return rc;
        }
        hipLaunchKernelGGL(student_pool_scatter_kernel, dim3(n, h->L), dim3(64), 0, s, h->pool_kv, h->pool_ring, h->pool_slot, 2 * D / 8, kv_layer,
                           (size_t)h->pool_S * h->F * 2 * D);
        HIP_OK(h, hipGetLastError());
        HIP_OK(h, h->pool_order.after_push(s));
        return 0;
    };
    if (int rc = enqueue()) {
        for (int i = 0; i < n; ++i) h->pool[(size_t)stream_ids[i]].reset(h->F);
        return rc;
    }
    pool_push_commit(h->pool, stream_ids, n);
    return 0;
}

int gitcap_student_pool_greedy(gitcap_student_t* h, const int32_t* stream_ids, int B, int max_len, int stop, int64_t* ids_out,
                               int32_t* steps_out, int32_t* frames_out, void* stream) {
    return greedy_entry(h, "student_pool_greedy", GREEDY_PARTS, OPT_FC, nullptr, max_len, stop, ids_out, steps_out, stream,
        [=](const StudentOpts&, const std::string& who, hipStream_t s, int* rows) { *rows = B; return pool_memory(h, who, stream_ids, B, s, frames_out); },
        !stream_ids);
}

// The beam form of the pool call: beam_entry over the pool's memory.  stream_ids and B are checked as gitcap_student_pool_greedy checks
// them (a null stream_ids is the family's "bad arguments"; B's range comes ahead of the family's checks so that it keeps its message).
int gitcap_student_pool_beam_search(gitcap_student_t* h, const int32_t* stream_ids, int B, int k, int max_len, int64_t* ids_out, void* stream) {
    const std::string who = "student_pool_beam_search";
    return beam_entry(h, who.c_str(), OPT_CO | OPT_PR | OPT_SO, OPT_FC, k, max_len, ids_out, stream,
        [&](int* clips) {
            *clips = B;
            if (!stream_ids) return fail(h, GITCAP_ERR_ARG, who + ": bad arguments");
            return B < 1 || B > h->R ? fail(h, GITCAP_ERR_ARG, who + ": B outside [1, max_rows]") : 0;
        },
        [&](const StudentOpts& o, hipStream_t s) { const int rc = beam_workspace(h, o.se.on); return rc ? rc : pool_memory(h, who, stream_ids, B, s, nullptr, k); });
}

int gitcap_student_pool_drop(gitcap_student_t* h, int stream_id) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "student_pool_drop: null handle");
    if (!h->pool_ring) return fail(h, GITCAP_ERR_STATE, "student_pool_drop: no pool (gitcap_student_pool_reset first)");
    if (stream_id < 0 || stream_id >= h->pool_S) return fail(h, GITCAP_ERR_ARG, "student_pool_drop: stream outside the pool");
    h->pool[(size_t)stream_id].reset(h->F);         // (what is in flight was enqueued with the old cursor; pool_order orders the next push)
    return 0;
}

int gitcap_student_pool_counts(const gitcap_student_t* h, int32_t* counts_out) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "student_pool_counts: null handle");
    if (!counts_out) return fail(h, GITCAP_ERR_ARG, "student_pool_counts: null counts_out");
    if (!h->pool_ring) return fail(h, GITCAP_ERR_STATE, "student_pool_counts: no pool (gitcap_student_pool_reset first)");
    for (int i = 0; i < h->pool_S; ++i) counts_out[i] = h->pool[(size_t)i].count;
    return 0;
}

}  // extern "C"
