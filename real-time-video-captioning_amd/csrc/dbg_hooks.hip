// libgitcap's handle-free test hooks: gitcap_dbg_* (but gitcap_dbg_config, which flips gitcap.hip's switches), gitcap_beam_topk*
// and gitcap_sample_rows*.  None touches a handle: each checks its arguments -- what a launcher does not check itself and a wrong
// value of which would index outside a buffer -- fills the launcher's record and calls ONE launcher on caller-owned device buffers.
// Declarations: include/gitcap.h.
#include "../../include/gitcap.h"
#include "kernels.h"
#include "host_logic.h"
#include "host_util.h"

#include <algorithm>
#include <cmath>
#include <mutex>
#include <vector>

extern "C" {

// ---- candidates of a search step (tests/test_selection_gpu.py, test_sampling_gpu.py, test_constraints_gpu.py) -----------------
static bool ban_mask_ok(const uint16_t* mask, int ld_mask, int V) {
    return mask && ((uintptr_t)mask & 3) == 0 && V > 0 && ld_mask >= (V + 15) / 16 && (ld_mask & 1) == 0;
}

// no handle here: the scratch of the two-stage top-k is a stream-ordered allocation
static int beam_topk_hook(const CandArgs& c, int K, void* stream) {
    if (!c.logits || !c.beam_scores || !c.out_scores || !c.out_idx || c.B <= 0 || c.beams <= 0 || c.V <= 0 || K <= 0) return GITCAP_ERR_ARG;
    void* scratch = nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (hipMallocAsync(&scratch, beam_topk_scratch_bytes(c.B, c.beams, c.V, K), s) != hipSuccess) return GITCAP_ERR_NOMEM;
    const hipError_t e = launch_beam_topk(c, K, scratch, s);
    (void)hipFreeAsync(scratch, s);
    return dbg_rc(e);
}
// the penalised forms: the penalty and its prefix, and the sizes before the scratch is sized
static bool topk_penalty_ok(const CandArgs& c, int K) {
    if (!(c.rp > 0.f) || !std::isfinite(c.rp)) return false;
    if (c.rp != 1.0f && (!c.prefix_ids || c.cur_len < 1 || c.ld_ids < c.cur_len || ((uintptr_t)c.prefix_ids & 7) != 0)) return false;
    return !(c.beams > 16 || K > 16 || (int64_t)K > (int64_t)c.beams * c.V || c.V > 131072);
}

int gitcap_beam_topk(const float* logits, int ld, const float* beam_scores, int B, int beams, int V, int K,
                     float* out_scores, int32_t* out_idx, void* stream) {
    return beam_topk_hook(CandArgs{logits, ld, beam_scores, nullptr, 0, 0, 1.0f, B, beams, V, out_scores, out_idx, nullptr}, K, stream);
}

int gitcap_beam_topk_penalized(const float* logits, int ld, const float* beam_scores, const int64_t* prefix_ids, int ld_ids, int cur_len,
                               float repetition_penalty, int B, int beams, int V, int K, float* out_scores, int32_t* out_idx, void* stream) {
    const CandArgs c{logits, ld, beam_scores, prefix_ids, ld_ids, cur_len, repetition_penalty, B, beams, V, out_scores, out_idx, nullptr};
    return topk_penalty_ok(c, K) ? beam_topk_hook(c, K, stream) : GITCAP_ERR_ARG;
}

int gitcap_beam_topk_constrained(const float* logits, int ld, const float* beam_scores, const int64_t* prefix_ids, int ld_ids, int cur_len,
                                 float repetition_penalty, int B, int beams, int V, int K, float* out_scores, int32_t* out_idx,
                                 const uint16_t* mask, int ld_mask, void* stream) {
    const HeadBan bn{mask, ld_mask};
    const CandArgs c{logits, ld, beam_scores, prefix_ids, ld_ids, cur_len, repetition_penalty, B, beams, V, out_scores, out_idx, &bn};
    return ban_mask_ok(mask, ld_mask, V) && topk_penalty_ok(c, K) ? beam_topk_hook(c, K, stream) : GITCAP_ERR_ARG;
}

static int sample_rows_hook(const CandArgs& c, int per_node, const SampleOpt& opt, const SampleStats& st, void* stream) {
    if (!c.logits || !c.beam_scores || !c.out_scores || !c.out_idx || c.B <= 0 || c.beams <= 0 || c.V <= 0 || per_node <= 0) return GITCAP_ERR_ARG;
    if (((uintptr_t)c.prefix_ids & 7) != 0 || ((uintptr_t)st.kept_out & 3) != 0 || ((uintptr_t)st.logz_out & 3) != 0) return GITCAP_ERR_ARG;
    return dbg_rc(launch_sample_rows(c, per_node, opt, st, (hipStream_t)stream));
}

int gitcap_sample_rows(const float* logits, int ld, const float* beam_scores, const int64_t* prefix_ids, int ld_ids, int cur_len,
                       float repetition_penalty, int B, int beams, int V, int per_node, float temperature, int top_k, float top_p,
                       uint64_t seed, float* out_scores, int32_t* out_idx, int32_t* kept_out, float* logz_out, void* stream) {
    const CandArgs c{logits, ld, beam_scores, prefix_ids, ld_ids, cur_len, repetition_penalty, B, beams, V, out_scores, out_idx, nullptr};
    return sample_rows_hook(c, per_node, SampleOpt{true, temperature, top_k, top_p, seed}, SampleStats{kept_out, logz_out}, stream);
}

int gitcap_sample_rows_constrained(const float* logits, int ld, const float* beam_scores, const int64_t* prefix_ids, int ld_ids, int cur_len,
                                   float repetition_penalty, int B, int beams, int V, int per_node, float temperature, int top_k, float top_p,
                                   uint64_t seed, float* out_scores, int32_t* out_idx, int32_t* kept_out, float* logz_out,
                                   const uint16_t* mask, int ld_mask, void* stream) {
    if (!ban_mask_ok(mask, ld_mask, V)) return GITCAP_ERR_ARG;
    const HeadBan bn{mask, ld_mask};
    const CandArgs c{logits, ld, beam_scores, prefix_ids, ld_ids, cur_len, repetition_penalty, B, beams, V, out_scores, out_idx, &bn};
    return sample_rows_hook(c, per_node, SampleOpt{true, temperature, top_k, top_p, seed}, SampleStats{kept_out, logz_out}, stream);
}

// ---- attention maps (tests/test_attention_map_gpu.py) -------------------------------------------------------------------------
int gitcap_dbg_attn_map(const gitcap_dbg_attn_map_args* d, void* stream) {
    if (!d || !d->kv_txt || !d->frame_mass || !d->text_mass) return GITCAP_ERR_ARG;
    if (d->L <= 0 || d->H <= 0 || d->rows <= 0 || d->rows_per_clip <= 0 || d->rows % d->rows_per_clip != 0 || d->T <= 0 || d->T > d->Tmax ||
        d->N < 0 || d->S_img < 0 || d->Smax < 0 || d->img_rows < 0)
        return GITCAP_ERR_ARG;
    if (!d->off && (int64_t)(d->rows / d->rows_per_clip) * d->S_img > d->img_rows) return GITCAP_ERR_ARG;
    if ((((uintptr_t)d->off | (uintptr_t)d->len | (uintptr_t)d->lengths | (uintptr_t)d->frame_mass | (uintptr_t)d->text_mass | (uintptr_t)d->patch_map) & 3) != 0)
        return GITCAP_ERR_ARG;
    AttnMapArgs a{};
    a.kv_img = (const bf16_t*)d->kv_img; a.img_layer_stride = (size_t)d->img_rows * 3 * d->D;
    a.kv_txt = (const bf16_t*)d->kv_txt; a.txt_layer_stride = (size_t)d->rows * d->Tmax * 3 * d->D;
    a.L = d->L; a.H = d->H; a.D = d->D; a.rows = d->rows; a.rows_per_clip = d->rows_per_clip; a.T = d->T; a.Tmax = d->Tmax;
    a.N = d->N; a.S_img = d->S_img; a.Smax = d->Smax; a.off = d->off; a.len = d->len; a.layer = d->layer; a.lengths = d->lengths;
    a.frame_mass = d->frame_mass; a.ld_f = d->ld_f; a.text_mass = d->text_mass; a.patch_map = d->patch_map; a.ld_s = d->ld_s;
    hipStream_t s = (hipStream_t)stream;
    void* scratch = nullptr;
    if (hipMallocAsync(&scratch, attn_map_scratch_floats(d->L, d->H, d->rows, d->T, d->layer) * sizeof(float), s) != hipSuccess) return GITCAP_ERR_NOMEM;
    a.stats = (float*)scratch;
    const hipError_t e = launch_attn_map(a, s);
    (void)hipFreeAsync(scratch, s);
    return dbg_rc(e);
}

// the student's read-out: cross_probs_kernel on caller-built q [M][H * hd] and memory keys k [rows][F][ldkv] (M = rows * T), then the
// head mean of that one layer -> frame_mass [rows][T][ld_f]; probs [M][H][F] is the caller's too
int gitcap_dbg_cross_probs(const void* q, const void* k, int ldkv, int rows, int T, int H, int hd, int F, const int32_t* lengths, float* probs,
                           float* frame_mass, int ld_f, void* stream) {
    if (!q || !k || !probs || !frame_mass || rows <= 0 || T <= 0 || H <= 0 || hd <= 0 || F <= 0 || ldkv < H * hd || (ldkv & 7) != 0 || ld_f < F ||
        (int64_t)rows * T * H * F > 0x7fffffff || (((uintptr_t)q | (uintptr_t)k) & 15) != 0 ||
        (((uintptr_t)probs | (uintptr_t)frame_mass | (uintptr_t)lengths) & 3) != 0)
        return GITCAP_ERR_ARG;
    const CrossProbsArgs a{(const bf16_t*)q, H * hd, T, (const bf16_t*)k, ldkv, F, F, probs, rows * T, H, hd};
    hipError_t e = launch_cross_probs(a, (hipStream_t)stream);
    if (e == hipSuccess) e = launch_cross_mean(probs, 1, rows, T, H, F, 0, lengths, frame_mass, ld_f, (hipStream_t)stream);
    return dbg_rc(e);
}

// its variable-length form (cross_probs_kernel<true>): k is PACKED, row r's keys are rows key_off[r] .. + key_len[r] - 1 of it (device
// int32 [rows] each); probs stays [M][H][F], zeros from key_len[r] on.  The tables are read back first (the call synchronises
// `stream`): a length outside [1, F] or a negative offset is refused before any launch.
int gitcap_dbg_cross_probs_varlen(const void* q, const void* k, int ldkv, int rows, int T, int H, int hd, int F, const int32_t* lengths, float* probs,
                                  float* frame_mass, int ld_f, const int32_t* key_off, const int32_t* key_len, void* stream) {
    if (!q || !k || !probs || !frame_mass || !key_off || !key_len || rows <= 0 || T <= 0 || H <= 0 || hd <= 0 || F <= 0 || F > 64 || ldkv < H * hd ||
        (ldkv & 7) != 0 || ld_f < F || (int64_t)rows * T * H * F > 0x7fffffff || (((uintptr_t)q | (uintptr_t)k) & 15) != 0 ||
        (((uintptr_t)probs | (uintptr_t)frame_mass | (uintptr_t)lengths | (uintptr_t)key_off | (uintptr_t)key_len) & 3) != 0)
        return GITCAP_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int32_t> tab(2 * (size_t)rows);
    if (hipStreamSynchronize(s) != hipSuccess || hipMemcpy(tab.data(), key_off, (size_t)rows * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(tab.data() + rows, key_len, (size_t)rows * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return GITCAP_ERR_HIP;
    for (int r = 0; r < rows; ++r)
        if (tab[r] < 0 || tab[rows + r] < 1 || tab[rows + r] > F) return GITCAP_ERR_ARG;
    const CrossProbsArgs a{(const bf16_t*)q, H * hd, T, (const bf16_t*)k, ldkv, F, F, probs, rows * T, H, hd};
    hipError_t e = launch_cross_probs_varlen(a, key_off, key_len, s);
    if (e == hipSuccess) e = launch_cross_mean(probs, 1, rows, T, H, F, 0, lengths, frame_mass, ld_f, s);
    return dbg_rc(e);
}

// ---- constrained decoding (tests/test_constraints_gpu.py) ---------------------------------------------------------------------
int gitcap_dbg_ban_mask(const int64_t* prefix_ids, int ld_ids, int rows, int cur_len, int n, int min_length, int sep_id,
                        const int32_t* suppress, int n_suppress, int V, uint16_t* mask_out, int ld_mask, void* stream) {
    if (((uintptr_t)prefix_ids & 7) != 0 || ((uintptr_t)suppress & 3) != 0) return GITCAP_ERR_ARG;
    return dbg_rc(launch_ban_mask(prefix_ids, ld_ids, rows, cur_len, n, min_length, sep_id, suppress, n_suppress, V, mask_out, ld_mask,
                                  (hipStream_t)stream));
}
// the form that reads its rules from a device record (kernels.h: launch_ban_mask_rec; tests/test_student_constraints_gpu.py)
int gitcap_dbg_ban_mask_rec(const int64_t* prefix_ids, int ld_ids, int rows, int cur_len, int sep_id, const int32_t* rec, int V,
                            uint16_t* mask_out, int ld_mask, void* stream) {
    if (((uintptr_t)prefix_ids & 7) != 0) return GITCAP_ERR_ARG;
    return dbg_rc(launch_ban_mask_rec(prefix_ids, ld_ids, rows, cur_len, sep_id, rec, V, mask_out, ld_mask, (hipStream_t)stream));
}

// ---- the student's prompted loops (tests/test_student_prompt_gpu.py) ---------------------------------------------------------------
int gitcap_dbg_student_prompt_stage(const int64_t* prompt_ids, int ld_prompt, const int32_t* lengths, int rows, int k, int max_len, int64_t cls,
                                    int64_t* ids, int ld, float* lp, int ld_lp, int pmin, void* stream) {
    if ((((uintptr_t)prompt_ids | (uintptr_t)ids) & 7) != 0 || (((uintptr_t)lengths | (uintptr_t)lp) & 3) != 0) return GITCAP_ERR_ARG;
    const StudentPromptStageArgs a{prompt_ids, ld_prompt, lengths, rows, k, max_len, cls, ids, ld, lp, ld_lp, pmin};
    return dbg_rc(launch_student_prompt_stage(a, (hipStream_t)stream));
}
// plain (prompt_ids null) and forced
int gitcap_dbg_student_beam_step(const float* cand_scores, const int32_t* cand_idx, const int64_t* ids_cur, int64_t* ids_next, float* scores,
                                 int32_t* src_rows, int B, int k, int V, int t, int ld, const int64_t* prompt_ids, int ld_prompt,
                                 const int32_t* lengths, int prompt_max_len, void* stream) {
    if ((((uintptr_t)ids_cur | (uintptr_t)ids_next | (uintptr_t)prompt_ids) & 7) != 0 || ((uintptr_t)lengths & 3) != 0) return GITCAP_ERR_ARG;
    const PromptArgs pr{prompt_ids, ld_prompt, lengths, 1, prompt_max_len};
    const StudentBeamStepArgs a{cand_scores, cand_idx, ids_cur, ids_next, scores, src_rows, B, k, V, t, ld, prompt_ids ? &pr : nullptr};
    return dbg_rc(launch_student_beam_step(a, (hipStream_t)stream));
}

int gitcap_dbg_gemm(const void* A, const void* W, const float* bias, const float* resid, void* out, int M, int N, int K,
                    int epi, int tile, void* stream) {
    GemmArgs a{};
    a.A = (const bf16_t*)A; a.lda = K; a.W = (const bf16_t*)W; a.bias = bias; a.M = M; a.N = N; a.K = K;
    a.out = out; a.ldo = N; a.resid = resid; a.ldr = N;
    if (epi < 0 || epi > EPI_BIAS_F32) return GITCAP_ERR_ARG;
    if (tile != 64 && tile != 128 && tile != 256) return GITCAP_ERR_ARG;
    const hipStream_t s = (hipStream_t)stream;
    hipError_t e = tile == 256 ? launch_gemm256(a, epi, s) : tile == 64 ? launch_gemm64(a, epi, s) : launch_gemm(a, epi, s);
    return e == hipSuccess ? 0 : GITCAP_ERR_HIP;
}

// fp8 tile kernel (gemm256.hip) on caller-owned buffers: A8 [M][K], W8 [N][K] e4m3 codes, wscale [N], acc * ascale * wscale[n] + bias;
// epi 4 -> out fp32 [M][N]; epi 0 -> bf16; epi 8 / 9 -> e4m3 codes of gelu(.) * out8_inv
int gitcap_dbg_gemm_f8(const void* A8, const void* W8, const float* wscale, float ascale, const float* bias, void* out, int M, int N,
                       int K, int epi, float out8_inv, void* stream) {
    GemmArgs a{};
    a.A = (const bf16_t*)A8; a.lda = K; a.W = (const bf16_t*)W8; a.wscale = wscale; a.ascale = ascale; a.bias = bias;
    a.M = M; a.N = N; a.K = K; a.out = out; a.ldo = N; a.out8_inv = out8_inv;
    if (epi != EPI_BIAS_F32 && epi != EPI_BIAS_BF16 && epi != EPI_BIAS_QGELU_F8 && epi != EPI_BIAS_GELU_F8) return GITCAP_ERR_ARG;
    if (!gemm256f8_ok(a)) return GITCAP_ERR_ARG;
    return launch_gemm256f8(a, epi, (hipStream_t)stream) == hipSuccess ? 0 : GITCAP_ERR_HIP;
}

// GEMM + bias [+ resid] + LayerNorm: fused = 1 the EPI_RESID_LN_* epilogue of the 256x256 kernel, 0 = GEMM (tile) then the
// row kernel; post as in gemm_ln (gitcap.hip).  out_f32: post ? LN(x) : x.  Scratch for the exchange is allocated here.
int gitcap_dbg_gemm_ln(const void* A, const void* W, const float* bias, const float* resid, const float* gamma,
                       const float* beta, float eps, float* out_f32, void* out_bf16, int M, int N, int K, int post,
                       int fused, int tile, void* stream) {
    static float2* stats = nullptr; static unsigned* cnt = nullptr; static int cap = 0;
    hipStream_t s = (hipStream_t)stream;
    GemmArgs a{};
    a.A = (const bf16_t*)A; a.lda = K; a.W = (const bf16_t*)W; a.bias = bias; a.M = M; a.N = N; a.K = K;
    a.out = out_f32; a.ldo = N; a.resid = resid; a.ldr = N;
    if (!fused) {
        if (tile != 64 && tile != 128 && tile != 256) return GITCAP_ERR_ARG;
        float* xo = out_f32;
        float* tmp = nullptr;
        if (post) { if (hipMalloc(&tmp, (size_t)M * N * 4) != hipSuccess) return GITCAP_ERR_NOMEM; xo = tmp; a.out = tmp; }
        const int epi = resid ? EPI_BIAS_RESID_F32 : EPI_BIAS_F32;
        hipError_t e = tile == 256 ? launch_gemm256(a, epi, s) : tile == 64 ? launch_gemm64(a, epi, s) : launch_gemm(a, epi, s);
        if (e == hipSuccess) {
            LnArgs l{xo, N, gamma, beta, eps, M, N, post ? out_f32 : nullptr, N, (bf16_t*)out_bf16, N, nullptr, 1, 1, nullptr, nullptr, 0.f};
            e = launch_layernorm(l, s);
        }
        if (tmp) { (void)hipStreamSynchronize(s); (void)hipFree(tmp); }
        return e == hipSuccess ? 0 : GITCAP_ERR_HIP;
    }
    if (M / 224 + 2 > cap) {
        if (stats) { (void)hipFree(stats); (void)hipFree(cnt); }
        cap = M / 224 + 2;
        if (hipMalloc(&stats, (size_t)cap * 256 * 16 * sizeof(float2)) != hipSuccess || hipMalloc(&cnt, (size_t)cap * 8) != hipSuccess) return GITCAP_ERR_NOMEM;
        if (hipMemset(cnt, 0, (size_t)cap * 8) != hipSuccess) return GITCAP_ERR_HIP;
    }
    a.ln_g = gamma; a.ln_b = beta; a.ln_eps = eps; a.ln_out = (bf16_t*)out_bf16; a.ld_ln = N; a.ln_stats = stats; a.ln_cnt = cnt;
    a.ln_stats_rows = cap * 224;
    const int epi = post ? EPI_RESID_LN_POST : EPI_RESID_LN_PRE;
    if (!post && !resid) return GITCAP_ERR_ARG;
    hipError_t e;
    if (fused != 1 || !gemm256_ln_ok(a)) return GITCAP_ERR_ARG;          // the 256x256 kernel of gemm256.hip
    e = launch_gemm256(a, epi, s);
    return e == hipSuccess ? 0 : GITCAP_ERR_HIP;
}

int gitcap_dbg_attn_full(const void* qkv, void* ctx, int G, int S, int H, void* stream) {
    return launch_attn_full((const bf16_t*)qkv, (bf16_t*)ctx, G, S, H, (hipStream_t)stream) == hipSuccess ? 0 : GITCAP_ERR_HIP;
}

int gitcap_dbg_layernorm(const float* x, const float* gamma, const float* beta, float eps, int rows, int D,
                         float* out_f32, void* out_bf16, void* stream) {
    LnArgs a{x, D, gamma, beta, eps, rows, D, out_f32, D, (bf16_t*)out_bf16, D, nullptr, 1, 1, nullptr, nullptr, 0.f};
    return launch_layernorm(a, (hipStream_t)stream) == hipSuccess ? 0 : GITCAP_ERR_HIP;
}

// ---- token selection (tests/test_selection_gpu.py) --------------------------------------------------------------------------
// launch_skinny with SK_BIAS_F32 under the identity row map: the vocabulary head of the token loops (switch 10 picks its form)
static SkinnyArgs dbg_head_args(const void* X, int ldx, const void* W, const float* wscale, const float* bias, int M, int N, int K,
                                float* logits, float* amax_val, int32_t* amax_idx, float* amax_sum) {
    SkinnyArgs a{};
    a.X = (const bf16_t*)X; a.ldx = ldx; a.W = W; a.wscale = wscale; a.bias = bias; a.M = M; a.N = N; a.K = K;
    a.out = logits; a.ldo = N; a.T = M; a.row_stride = M; a.row_off = 0;
    a.amax_val = amax_val; a.amax_idx = amax_idx; a.Wpk = nullptr; a.amax_sum = amax_sum;
    return a;
}
static int dbg_vocab_head(const SkinnyArgs& a, void* stream, const HeadTargets* tg = nullptr, const HeadBan* bn = nullptr) {
    if (!a.X || !a.W || a.M <= 0 || a.N <= 0 || a.ldx < a.K || a.ldx % 8 || !skinny_full_ok(a.K) || (a.amax_val == nullptr) != (a.amax_idx == nullptr) ||
        (!a.out && !a.amax_val) || (a.amax_sum && !a.amax_val))
        return GITCAP_ERR_ARG;
    return dbg_rc(launch_skinny(a, SK_BIAS_F32, (hipStream_t)stream, tg, bn));
}
int gitcap_dbg_vocab_head(const void* X, int ldx, const void* W, const float* wscale, const float* bias, int M, int N, int K,
                          float* logits, float* amax_val, int32_t* amax_idx, void* stream) {
    return dbg_vocab_head(dbg_head_args(X, ldx, W, wscale, bias, M, N, K, logits, amax_val, amax_idx, nullptr), stream);
}
// the same launch with the third partial (amax_sum [M][ntiles], required)
int gitcap_dbg_vocab_head_lse(const void* X, int ldx, const void* W, const float* wscale, const float* bias, int M, int N, int K,
                              float* logits, float* amax_val, int32_t* amax_idx, float* amax_sum, void* stream) {
    if (!amax_sum) return GITCAP_ERR_ARG;
    return dbg_vocab_head(dbg_head_args(X, ldx, W, wscale, bias, M, N, K, logits, amax_val, amax_idx, amax_sum), stream);
}
// the BAN forms of the same launch (mask uint16 [M][ld_mask], kernels.h: HeadBan); amax_sum NULL: the plain form, else the LSE form
int gitcap_dbg_vocab_head_banned(const void* X, int ldx, const void* W, const float* wscale, const float* bias, int M, int N, int K,
                                 float* logits, float* amax_val, int32_t* amax_idx, float* amax_sum, const uint16_t* mask, int ld_mask,
                                 void* stream) {
    if (!ban_mask_ok(mask, ld_mask, N)) return GITCAP_ERR_ARG;
    const HeadBan bn{mask, ld_mask};
    return dbg_vocab_head(dbg_head_args(X, ldx, W, wscale, bias, M, N, K, logits, amax_val, amax_idx, amax_sum), stream, nullptr, &bn);
}
// the scoring head: the _lse launch + the logit of each row's target column (targets int64 [M], tgt_logit fp32 [M])
int gitcap_dbg_vocab_head_score(const void* X, int ldx, const void* W, const float* wscale, const float* bias, int M, int N, int K,
                                float* logits, float* amax_val, int32_t* amax_idx, float* amax_sum, const int64_t* targets, float* tgt_logit,
                                void* stream) {
    if (!amax_val || !amax_idx || !amax_sum || !targets || !tgt_logit) return GITCAP_ERR_ARG;
    const HeadTargets tg{targets, M, M, 0, tgt_logit};
    return dbg_vocab_head(dbg_head_args(X, ldx, W, wscale, bias, M, N, K, logits, amax_val, amax_idx, amax_sum), stream, &tg);
}
// launch_head_topk with its head (tests/test_top_logprobs_gpu.py): the LSE head over the M rows (ban_mask set: its BAN form), then
// the k best columns of every row -> top_ids / top_lp [M][k].  W [ceil(V / 16) * 16][D] (bf16, or e4m3 codes with wscale), Wpk
// nullable = its fragment-major copy.  No handle: the three partials are a stream-ordered allocation.
int gitcap_dbg_head_topk(const void* X, int ldx, int M, const void* W, const void* Wpk, const float* wscale, const float* bias, int V, int D,
                         int k, const uint16_t* ban_mask, int ld_mask, int64_t* top_ids, float* top_lp, void* stream) {
    if (!X || !W || M <= 0 || V <= 0 || !head_topk_ok(D, wscale != nullptr) || (ban_mask && !ban_mask_ok(ban_mask, ld_mask, V)))
        return GITCAP_ERR_ARG;
    const size_t n = (size_t)M * ((V + 15) / 16);
    float* part = nullptr;
    hipStream_t s = (hipStream_t)stream;
    if (hipMallocAsync((void**)&part, 3 * n * 4, s) != hipSuccess) return GITCAP_ERR_NOMEM;
    const HeadBan bn{ban_mask, ld_mask};
    HeadTopkArgs a{};
    a.X = (const bf16_t*)X; a.ldx = ldx; a.hw = HeadWeight{W, Wpk, wscale, bias, V, D};
    a.val = part; a.idx = (int*)(part + n); a.sum = part + 2 * n; a.bn = ban_mask ? &bn : nullptr; a.run_head = true; a.M = M;
    a.rows = M; a.T = 1; a.row_stride = 1; a.row_off = 0; a.k = k; a.top_ids = top_ids; a.top_lp = top_lp; a.ld = 1;
    const hipError_t e = launch_head_topk(a, s);
    (void)hipFreeAsync(part, s);
    return dbg_rc(e);
}
// launch_score_final on caller-owned buffers: partials [rows * T][ntiles], tgt_logit [rows * T], ids [rows][ld_ids]
int gitcap_dbg_score_final(const float* amax_val, const int32_t* amax_idx, const float* amax_sum, int ntiles, const float* tgt_logit,
                           const int64_t* ids, int ld_ids, int rows, int T, const int32_t* lengths, int64_t ignore_id, int V,
                           float* token_lp, int ld_lp, float* row_sum, int32_t* row_cnt, int64_t* top1_ids, float* top1_lp, void* stream) {
    if (!token_lp) return GITCAP_ERR_ARG;
    const ScoreOut o{token_lp, ld_lp, row_sum, row_cnt, top1_ids, top1_lp};
    return dbg_rc(launch_score_final(amax_val, amax_idx, amax_sum, ntiles, tgt_logit, ids, ld_ids, rows, T, lengths, ignore_id, V, o,
                                     (hipStream_t)stream));
}

// launch_head_dual on caller-owned buffers, row-major weights; targets: one column per row (HeadTargets with T = ld = M, shift 0)
int gitcap_dbg_vocab_head_dual(const void* Xt, int ldxt, const void* Wt, const float* wscale, const float* bias_t, int Kt, const void* Xs,
                               int ldxs, const void* Ws, const float* bias_s, int Ks, int M, int N, float inv_temperature, float* t_max,
                               int32_t* t_idx, float* t_sum, float* s_max, int32_t* s_idx, float* s_sum, float* cross,
                               const int64_t* targets, float* t_logit, float* s_logit, void* stream) {
    DualHeadArgs a{};
    a.Xt = (const bf16_t*)Xt; a.ldxt = ldxt; a.Xs = (const bf16_t*)Xs; a.ldxs = ldxs;
    a.wt = HeadWeight{Wt, nullptr, wscale, bias_t, N, Kt}; a.ws = HeadWeight{Ws, nullptr, nullptr, bias_s, N, Ks};
    a.M = M; a.inv_temp = inv_temperature;
    a.t_max = t_max; a.t_idx = t_idx; a.t_sum = t_sum; a.s_max = s_max; a.s_idx = s_idx; a.s_sum = s_sum; a.cross = cross;
    if (targets) { a.tg = HeadTargets{targets, M, M, 0, t_logit}; a.s_logit = s_logit; }
    return dbg_rc(launch_head_dual(a, (hipStream_t)stream));
}
int gitcap_dbg_distill_final(const float* t_max, const int32_t* t_idx, const float* t_sum, const float* s_max, const int32_t* s_idx,
                             const float* s_sum, const float* cross, int ntiles, const float* t_logit, const float* s_logit,
                             const int64_t* ids, int ld_ids, int rows, int T, const int32_t* lengths, int64_t ignore_id, int V,
                             const gitcap_distill_out* out, void* stream) {
    if (!out) return GITCAP_ERR_ARG;
    const DistillOut o{out->kl, out->ld_kl, out->teacher_top1, out->student_top1, out->agree, out->teacher_lp, out->student_lp, out->ld_lp,
                       out->row_kl_sum, out->row_cnt};
    return dbg_rc(launch_distill_final(DistillPartials{t_max, t_idx, t_sum, s_max, s_idx, s_sum, cross}, ntiles, t_logit, s_logit, ids, ld_ids,
                                       rows, T, lengths, ignore_id, V, o, (hipStream_t)stream));
}

// launch_argmax_final: the arguments every form shares; a form adds its own (sum / lp_out, prompt) before dbg_argmax_final
static ArgmaxArgs dbg_argmax_args(const float* amax_val, const int32_t* amax_idx, int ntiles, int rows, int row_stride, int row_off,
                                  int64_t* out, int ld_out, int32_t* sep_cnt, int step, int sep_id) {
    ArgmaxArgs a{};
    a.val = amax_val; a.idx = amax_idx; a.ntiles = ntiles; a.rows = rows; a.row_stride = row_stride; a.row_off = row_off;
    a.out = out; a.ld_out = ld_out; a.sep_cnt = sep_cnt; a.step = step; a.sep_id = sep_id;
    a.prompt_pos = step + 1;              // the position a forced launch writes
    return a;
}
static int dbg_argmax_final(ArgmaxArgs a, const gitcap_dbg_next_embed* emb, void* stream) {
    if (!a.val || !a.idx || !a.out || a.ntiles <= 0 || a.rows <= 0 || a.row_stride <= 0 || a.row_off < 0 || a.ld_out <= 0 || a.step < 0)
        return GITCAP_ERR_ARG;
    NextEmbed ne{};
    if (emb) {
        if (emb->vocab <= 0 || emb->position < 0) return GITCAP_ERR_ARG;
        ne = NextEmbed{emb->word, emb->pos, emb->gamma, emb->beta, emb->eps, emb->D, emb->vocab, emb->position, emb->xf, (bf16_t*)emb->xb};
        a.emb = &ne;
    }
    return dbg_rc(launch_argmax_final(a, (hipStream_t)stream));
}
int gitcap_dbg_argmax_final(const float* amax_val, const int32_t* amax_idx, int ntiles, int rows, int row_stride, int row_off,
                            int64_t* out, int ld_out, int32_t* sep_cnt, int step, int sep_id, const gitcap_dbg_next_embed* emb,
                            void* stream) {
    return dbg_argmax_final(dbg_argmax_args(amax_val, amax_idx, ntiles, rows, row_stride, row_off, out, ld_out, sep_cnt, step, sep_id), emb, stream);
}
int gitcap_dbg_argmax_final_lp(const float* amax_val, const int32_t* amax_idx, int ntiles, int rows, int row_stride, int row_off,
                               int64_t* out, int ld_out, int32_t* sep_cnt, int step, int sep_id, const gitcap_dbg_next_embed* emb,
                               const float* amax_sum, float* lp_out, int ld_lp, void* stream) {
    if (!amax_sum || !lp_out || ld_lp < 1) return GITCAP_ERR_ARG;
    ArgmaxArgs a = dbg_argmax_args(amax_val, amax_idx, ntiles, rows, row_stride, row_off, out, ld_out, sep_cnt, step, sep_id);
    a.sum = amax_sum; a.lp_out = lp_out; a.ld_lp = ld_lp;
    return dbg_argmax_final(a, emb, stream);
}
// the forced form (gitcap_attach_prompt): the launch writes position step + 1; amax_sum / lp_out both or neither
int gitcap_dbg_argmax_final_forced(const float* amax_val, const int32_t* amax_idx, int ntiles, int rows, int row_stride, int row_off,
                                   int64_t* out, int ld_out, int32_t* sep_cnt, int step, int sep_id, const gitcap_dbg_next_embed* emb,
                                   const float* amax_sum, float* lp_out, int ld_lp, const int64_t* prompt_ids, int ld_prompt,
                                   const int32_t* lengths, int max_len, void* stream) {
    if (!prompt_ids || !lengths || max_len < 1 || ld_prompt < max_len || (amax_sum == nullptr) != (lp_out == nullptr) || (lp_out && ld_lp < 1))
        return GITCAP_ERR_ARG;
    const PromptArgs pr{prompt_ids, ld_prompt, lengths, 1, max_len};
    ArgmaxArgs a = dbg_argmax_args(amax_val, amax_idx, ntiles, rows, row_stride, row_off, out, ld_out, sep_cnt, step, sep_id);
    a.sum = amax_sum; a.lp_out = lp_out; a.ld_lp = ld_lp; a.prompt = &pr;
    return dbg_argmax_final(a, emb, stream);
}

// launch_draft_accept: the two words the kernel publishes go through a page-locked int32[2] this hook owns (made once, kept for
// the process) and, with lp_out, the tokens through a device int[B * n] scratch this hook owns as well
static int dbg_draft_accept(DraftAcceptArgs a, int32_t* host_out, void* stream) {
    static std::mutex mu;
    static int32_t* host = nullptr;
    static int* lp_tok = nullptr;
    static int64_t lp_cap = 0;
    if (!host_out) return GITCAP_ERR_ARG;
    std::lock_guard<std::mutex> lock(mu);
    if (!host && hipHostMalloc((void**)&host, 16, hipHostMallocMapped) != hipSuccess) { host = nullptr; return GITCAP_ERR_NOMEM; }
    if (a.lp_out && a.B > 0 && a.n > 0 && (int64_t)a.B * a.n > lp_cap) {
        if (lp_tok) { (void)hipDeviceSynchronize(); (void)hipFree(lp_tok); }
        lp_cap = std::max<int64_t>((int64_t)a.B * a.n, 1024);
        if (hipMalloc((void**)&lp_tok, (size_t)lp_cap * 4) != hipSuccess) { lp_tok = nullptr; lp_cap = 0; return GITCAP_ERR_NOMEM; }
    }
    const hipStream_t s = (hipStream_t)stream;
    ((volatile int32_t*)host)[0] = -1;
    ((volatile int32_t*)host)[1] = -1;
    a.host = host; a.lp_tok = a.lp_out ? lp_tok : nullptr;
    const hipError_t e = launch_draft_accept(a, s);
    if (e != hipSuccess) return dbg_rc(e);
    if (hipStreamSynchronize(s) != hipSuccess) return GITCAP_ERR_HIP;
    host_out[0] = ((volatile int32_t*)host)[0];
    host_out[1] = ((volatile int32_t*)host)[1];
    return 0;
}
int gitcap_dbg_draft_accept_lp(const float* amax_val, const int32_t* amax_idx, int ntiles, int B, int n, int64_t* ids, int ld, int32_t* tok,
                               uint32_t* ticket, int32_t* sep_cnt, int sep_id, int32_t* host_out, const float* amax_sum, float* lp_out,
                               int ld_lp, void* stream) {
    if (!amax_sum || !lp_out || ld_lp < 1) return GITCAP_ERR_ARG;
    DraftAcceptArgs a{};
    a.val = amax_val; a.idx = amax_idx; a.sum = amax_sum; a.ntiles = ntiles; a.B = B; a.n = n; a.ids = ids; a.ld = ld; a.tok = tok;
    a.ticket = ticket; a.sep_cnt = sep_cnt; a.sep_id = sep_id; a.lp_out = lp_out; a.ld_lp = ld_lp;
    return dbg_draft_accept(a, host_out, stream);
}
int gitcap_dbg_draft_accept(const float* amax_val, const int32_t* amax_idx, int ntiles, int B, int n, int64_t* ids, int ld, int32_t* tok,
                            uint32_t* ticket, int32_t* sep_cnt, int sep_id, int32_t* host_out, void* stream) {
    DraftAcceptArgs a{};
    a.val = amax_val; a.idx = amax_idx; a.ntiles = ntiles; a.B = B; a.n = n; a.ids = ids; a.ld = ld; a.tok = tok;
    a.ticket = ticket; a.sep_cnt = sep_cnt; a.sep_id = sep_id;
    return dbg_draft_accept(a, host_out, stream);
}

// the kept form (a verified draft's tail): the launch writes position step + 1; amax_sum / lp_out both or neither
int gitcap_dbg_argmax_final_keep(const float* amax_val, const int32_t* amax_idx, int ntiles, int rows, int row_stride, int row_off,
                                 int64_t* out, int ld_out, int32_t* sep_cnt, int step, int sep_id, const gitcap_dbg_next_embed* emb,
                                 const float* amax_sum, float* lp_out, int ld_lp, const int32_t* len, void* stream) {
    if (!len || (amax_sum == nullptr) != (lp_out == nullptr) || (lp_out && ld_lp < 1)) return GITCAP_ERR_ARG;
    ArgmaxArgs a = dbg_argmax_args(amax_val, amax_idx, ntiles, rows, row_stride, row_off, out, ld_out, sep_cnt, step, sep_id);
    a.sum = amax_sum; a.lp_out = lp_out; a.ld_lp = ld_lp; a.keep_len = len;
    return dbg_argmax_final(a, emb, stream);
}

// launch_draft_accept_rows: the words the kernel publishes go through a page-locked int32[4 + B] this hook owns and, with lp_out,
// the log-probabilities through a device int[B * n] scratch this hook owns as well
static int dbg_draft_accept_rows(DraftAcceptRowsArgs a, int32_t* host_out, void* stream) {
    static std::mutex mu;
    static int32_t* host = nullptr;
    static int64_t host_cap = 0;
    static int* lp_tok = nullptr;
    static int64_t lp_cap = 0;
    if (!host_out || a.B <= 0 || a.n <= 0) return GITCAP_ERR_ARG;
    std::lock_guard<std::mutex> lock(mu);
    if (4 + (int64_t)a.B > host_cap) {
        if (host) { (void)hipDeviceSynchronize(); (void)hipHostFree(host); }
        host_cap = std::max<int64_t>(4 + (int64_t)a.B, 1024);
        if (hipHostMalloc((void**)&host, (size_t)host_cap * 4, hipHostMallocMapped) != hipSuccess) { host = nullptr; host_cap = 0; return GITCAP_ERR_NOMEM; }
    }
    if (a.lp_out && (int64_t)a.B * a.n > lp_cap) {
        if (lp_tok) { (void)hipDeviceSynchronize(); (void)hipFree(lp_tok); }
        lp_cap = std::max<int64_t>((int64_t)a.B * a.n, 1024);
        if (hipMalloc((void**)&lp_tok, (size_t)lp_cap * 4) != hipSuccess) { lp_tok = nullptr; lp_cap = 0; return GITCAP_ERR_NOMEM; }
    }
    const hipStream_t s = (hipStream_t)stream;
    for (int i = 0; i < 4 + a.B; ++i) ((volatile int32_t*)host)[i] = -1;
    a.host = host; a.host_rows = host + 4; a.lp_tok = a.lp_out ? lp_tok : nullptr;
    const hipError_t e = launch_draft_accept_rows(a, s);
    if (e != hipSuccess) return dbg_rc(e);
    if (hipStreamSynchronize(s) != hipSuccess) return GITCAP_ERR_HIP;
    for (int i = 0; i < 4 + a.B; ++i) host_out[i] = ((volatile int32_t*)host)[i];
    return 0;
}
static DraftAcceptRowsArgs dbg_accept_rows_args(const float* amax_val, const int32_t* amax_idx, int ntiles, int B, int n, int64_t* ids, int ld,
                                                int32_t* len, int32_t* tok, int32_t* row_res, uint32_t* ticket, int32_t* sep_cnt, int sep_id) {
    DraftAcceptRowsArgs a{};
    a.val = amax_val; a.idx = amax_idx; a.ntiles = ntiles; a.B = B; a.n = n; a.ids = ids; a.ld = ld; a.len = len; a.tok = tok;
    a.row_res = row_res; a.ticket = ticket; a.sep_cnt = sep_cnt; a.sep_id = sep_id;
    return a;
}
int gitcap_dbg_draft_accept_rows(const float* amax_val, const int32_t* amax_idx, int ntiles, int B, int n, int64_t* ids, int ld,
                                 int32_t* len, int32_t* tok, int32_t* row_res, uint32_t* ticket, int32_t* sep_cnt, int sep_id,
                                 int32_t* host_out, void* stream) {
    return dbg_draft_accept_rows(dbg_accept_rows_args(amax_val, amax_idx, ntiles, B, n, ids, ld, len, tok, row_res, ticket, sep_cnt, sep_id),
                                 host_out, stream);
}
int gitcap_dbg_draft_accept_rows_lp(const float* amax_val, const int32_t* amax_idx, int ntiles, int B, int n, int64_t* ids, int ld,
                                    int32_t* len, int32_t* tok, int32_t* row_res, uint32_t* ticket, int32_t* sep_cnt, int sep_id,
                                    int32_t* host_out, const float* amax_sum, float* lp_out, int ld_lp, void* stream) {
    if (!amax_sum || !lp_out || ld_lp < 1) return GITCAP_ERR_ARG;
    DraftAcceptRowsArgs a = dbg_accept_rows_args(amax_val, amax_idx, ntiles, B, n, ids, ld, len, tok, row_res, ticket, sep_cnt, sep_id);
    a.sum = amax_sum; a.lp_out = lp_out; a.ld_lp = ld_lp;
    return dbg_draft_accept_rows(a, host_out, stream);
}

static bool dbg_beam_buffers(const gitcap_dbg_beam_buffers* b, BeamBuffers& bb) {
    if (!b || !b->ids0 || !b->ids1 || !b->words || !b->hyp_ids || !b->beam_scores || !b->hyp_score || !b->src_rows || !b->done || !b->hyp_len)
        return false;
    bb = BeamBuffers{b->ids0, b->ids1, b->words, b->hyp_ids, b->beam_scores, b->hyp_score, b->src_rows, b->done, b->hyp_len};
    return true;
}

// (gitcap_dbg_beam_buffers_nbest is gitcap_dbg_beam_buffers with the slot count n behind it)
static bool dbg_beam_buffers_nbest(const gitcap_dbg_beam_buffers_nbest* b, BeamBuffers& bb) {
    if (!b || b->n < 1 || b->n > 16) return false;
    const gitcap_dbg_beam_buffers first{b->ids0, b->ids1, b->words, b->hyp_ids, b->beam_scores, b->hyp_score, b->src_rows, b->done, b->hyp_len};
    return dbg_beam_buffers(&first, bb);
}

int gitcap_dbg_beam_init(const gitcap_dbg_beam_buffers* b, int B, int beams, int max_len, int cls, void* stream) {
    BeamBuffers bb;
    if (!dbg_beam_buffers(b, bb) || B <= 0 || beams <= 0 || beams > 16 || max_len < 2) return GITCAP_ERR_ARG;
    return dbg_rc(launch_beam_init(bb, B, beams, 1, max_len, cls, (hipStream_t)stream));
}

int gitcap_dbg_beam_finish(const gitcap_dbg_beam_buffers* b, int B, int max_len, int eos, int64_t* decoded, float* logprobs, void* stream) {
    BeamBuffers bb;
    if (!dbg_beam_buffers(b, bb) || !decoded || !logprobs || B <= 0 || max_len < 2) return GITCAP_ERR_ARG;
    return dbg_rc(launch_beam_finish(bb, 1, B, max_len, eos, BeamFinishOut{decoded, logprobs, nullptr, nullptr}, (hipStream_t)stream));
}

int gitcap_dbg_beam_finish_nbest(const gitcap_dbg_beam_buffers_nbest* b, int B, int max_len, int eos, int64_t* decoded, float* logprobs,
                                 void* stream) {
    BeamBuffers bb;
    if (!dbg_beam_buffers_nbest(b, bb) || !decoded || !logprobs || B <= 0 || max_len < 2) return GITCAP_ERR_ARG;
    return dbg_rc(launch_beam_finish(bb, b->n, B, max_len, eos, BeamFinishOut{decoded, logprobs, nullptr, nullptr}, (hipStream_t)stream));
}

// launch_beam_step: one body for every form (the launcher refuses beams > 16 and K > 16 with the same status)
static int dbg_beam_step(const BeamBuffers& bb, const BeamStepArgs& a, void* stream) {
    if (!a.cand_scores || !a.cand_idx || a.B <= 0 || a.beams <= 0 || a.beams > 16 || a.K <= 0 || a.K > 16 || a.V <= 0 || a.cur_len < 1 ||
        a.cur_len >= a.max_len || (a.cur != 0 && a.cur != 1))
        return GITCAP_ERR_ARG;
    return dbg_rc(launch_beam_step(bb, a, (hipStream_t)stream));
}
// the n-slot buffers' forms: a.n is the buffers'
static int dbg_beam_step_nbest(const gitcap_dbg_beam_buffers_nbest* b, BeamStepArgs a, void* stream) {
    BeamBuffers bb;
    if (!dbg_beam_buffers_nbest(b, bb)) return GITCAP_ERR_ARG;
    a.n = b->n;
    return dbg_beam_step(bb, a, stream);
}

int gitcap_dbg_beam_step(const gitcap_dbg_beam_buffers* b, const float* cand_scores, const int32_t* cand_idx, int B, int beams, int K,
                         int V, int cur_len, int max_len, int eos, float length_penalty, int cur, void* stream) {
    BeamBuffers bb;
    if (!dbg_beam_buffers(b, bb)) return GITCAP_ERR_ARG;
    return dbg_beam_step(bb, BeamStepArgs{1, cand_scores, cand_idx, B, beams, K, V, cur_len, max_len, eos, length_penalty, cur, false, nullptr}, stream);
}

int gitcap_dbg_beam_step_nbest(const gitcap_dbg_beam_buffers_nbest* b, const float* cand_scores, const int32_t* cand_idx, int B, int beams,
                               int K, int V, int cur_len, int max_len, int eos, float length_penalty, int cur, void* stream) {
    return dbg_beam_step_nbest(b, BeamStepArgs{0, cand_scores, cand_idx, B, beams, K, V, cur_len, max_len, eos, length_penalty, cur, false, nullptr}, stream);
}

int gitcap_dbg_beam_step_sampled(const gitcap_dbg_beam_buffers_nbest* b, const float* cand_scores, const int32_t* cand_idx, int B, int beams,
                                 int K, int V, int cur_len, int max_len, int eos, float length_penalty, int cur, void* stream) {
    return dbg_beam_step_nbest(b, BeamStepArgs{0, cand_scores, cand_idx, B, beams, K, V, cur_len, max_len, eos, length_penalty, cur, true, nullptr}, stream);
}

// the forced forms (gitcap_attach_prompt): sampled = 0 and n = 1 runs beam_step_kernel, n > 1 the n-slot kernel, sampled != 0 its form
// for draws; prompt_ids [B][ld_prompt], lengths [B], prompt_max_len < max_len
int gitcap_dbg_beam_step_forced(const gitcap_dbg_beam_buffers_nbest* b, const float* cand_scores, const int32_t* cand_idx, int B, int beams,
                                int K, int V, int cur_len, int max_len, int eos, float length_penalty, int cur, int sampled,
                                const int64_t* prompt_ids, int ld_prompt, const int32_t* lengths, int prompt_max_len, void* stream) {
    if (!prompt_ids || !lengths || prompt_max_len < 1 || prompt_max_len >= max_len || ld_prompt < prompt_max_len) return GITCAP_ERR_ARG;
    const PromptArgs pr{prompt_ids, ld_prompt, lengths, 1, prompt_max_len};
    return dbg_beam_step_nbest(b, BeamStepArgs{0, cand_scores, cand_idx, B, beams, K, V, cur_len, max_len, eos, length_penalty, cur, sampled != 0, &pr}, stream);
}

// ---- text-row kernels of the token loop (tests/test_text_rows_gpu.py): each hook is ONE launcher on caller-owned device buffers,
// no allocation, no handle; what a launcher does not check itself and a wrong value of which would index outside a buffer is
// checked here
int gitcap_dbg_pack_frags(const void* src, void* dst, int rows16, int K, int elem_bytes, void* stream) {
    if (!src || !dst || K <= 0 || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return GITCAP_ERR_ARG;
    return dbg_rc(launch_pack_frags(src, dst, rows16, K, elem_bytes, (hipStream_t)stream));
}

int gitcap_dbg_kv_quant_v(const void* kv, void* v8, float* vs, int rows, int D, int H, int64_t pitch, void* stream) {
    if (!kv || !v8 || !vs || H <= 0 || ((uintptr_t)kv & 15) || ((uintptr_t)v8 & 7)) return GITCAP_ERR_ARG;
    return dbg_rc(launch_kv_quant_v((const bf16_t*)kv, (unsigned char*)v8, vs, rows, D, H, pitch, (hipStream_t)stream));
}

int gitcap_dbg_skinny(const gitcap_dbg_skinny_args* g, int epi, void* stream) {
    if (!g || !g->W || !g->out || g->M <= 0 || g->N <= 0 || !skinny_full_ok(g->K) || g->ldo < g->N || g->T <= 0 || g->row_stride < 0 ||
        g->row_off < 0 || ((uintptr_t)g->W & 15) || ((uintptr_t)g->Wpk & 15) || ((uintptr_t)g->out & 7) || (g->ldo & 3))
        return GITCAP_ERR_ARG;
    if (epi != SK_BIAS_BF16 && epi != SK_BIAS_GELU_BF16 && epi != SK_BIAS_RELU_BF16) return GITCAP_ERR_ARG;   // the head: gitcap_dbg_vocab_head
    if (g->wscale && g->K != 128 && g->K != 768) return GITCAP_ERR_ARG;
    SkinnyArgs a{};
    a.X = (const bf16_t*)g->X; a.ldx = g->ldx; a.W = g->W; a.Wpk = g->Wpk; a.wscale = g->wscale; a.bias = g->bias;
    a.M = g->M; a.N = g->N; a.K = g->K; a.out = g->out; a.ldo = g->ldo; a.T = g->T; a.row_stride = g->row_stride; a.row_off = g->row_off;
    if (g->ln_kind) {
        if ((g->ln_kind != 1 && g->ln_kind != 2) || !skinny_row_prologue_ok(g->M, g->K, g->wscale != nullptr) || epi == SK_BIAS_GELU_BF16 ||
            !g->ln_g || !g->ln_b || !g->ln_xf)
            return GITCAP_ERR_ARG;
        if (g->ln_kind == 1 && (!g->ln_slabs || g->ln_nslab <= 0 || !g->ln_bias || !g->ln_resid || g->ln_resid == g->ln_xf)) return GITCAP_ERR_ARG;
        if (g->ln_kind == 2 && (!g->ln_ids || g->ln_T <= 0 || g->ln_ld_ids < g->ln_T || g->ln_t0 < 0 || g->ln_vocab <= 0 || !g->ln_word || !g->ln_pos))
            return GITCAP_ERR_ARG;
        a.ln.kind = g->ln_kind; a.ln.slabs = g->ln_slabs; a.ln.nslab = g->ln_nslab; a.ln.bias = g->ln_bias; a.ln.resid = g->ln_resid;
        a.ln.ids = g->ln_ids; a.ln.ld_ids = g->ln_ld_ids; a.ln.T = g->ln_T; a.ln.t0 = g->ln_t0; a.ln.vocab = g->ln_vocab;
        a.ln.word = g->ln_word; a.ln.pos = g->ln_pos; a.ln.g = g->ln_g; a.ln.b = g->ln_b; a.ln.eps = g->ln_eps; a.ln.xf = g->ln_xf;
    } else if (!g->X || g->ldx < g->K || (g->ldx & 7) || ((uintptr_t)g->X & 15)) {
        return GITCAP_ERR_ARG;
    }
    return dbg_rc(launch_skinny(a, epi, (hipStream_t)stream));
}

int gitcap_dbg_skinny_splitk(const void* X, int ldx, const void* W, const void* Wpk, const float* wscale, int M, int N, int K, int ksplit,
                             float* slabs, int ldo, void* stream) {
    if (!X || !W || !slabs || M <= 0 || N <= 0 || K <= 0 || ksplit < 0 || ldx < K || (ldx & 7) || ldo < N || (ldo & 3) ||
        ((uintptr_t)X & 15) || ((uintptr_t)W & 15) || ((uintptr_t)Wpk & 15) || ((uintptr_t)slabs & 15))
        return GITCAP_ERR_ARG;
    SkinnyArgs a{};
    a.X = (const bf16_t*)X; a.ldx = ldx; a.W = W; a.Wpk = Wpk; a.wscale = wscale; a.M = M; a.N = N; a.K = K;
    a.out = slabs; a.ldo = ldo; a.T = M; a.row_stride = M; a.ksplit = ksplit;
    return dbg_rc(launch_skinny_splitk(a, (hipStream_t)stream));
}

int gitcap_dbg_ln_reduce(const float* slabs, int nslab, const float* bias, const float* resid, const float* gamma, const float* beta,
                         float eps, int M, int D, float* xf, void* xb, void* stream) {
    if (!slabs || !bias || !resid || !gamma || !beta || !xf || !xb || M <= 0 || D <= 0 || (D & 3) || nslab <= 0) return GITCAP_ERR_ARG;
    if (((uintptr_t)slabs & 15) || ((uintptr_t)bias & 15) || ((uintptr_t)resid & 15) || ((uintptr_t)gamma & 15) || ((uintptr_t)beta & 15) ||
        ((uintptr_t)xf & 15) || ((uintptr_t)xb & 7))
        return GITCAP_ERR_ARG;
    return dbg_rc(launch_ln_reduce(slabs, nslab, bias, resid, gamma, beta, eps, M, D, xf, (bf16_t*)xb, (hipStream_t)stream));
}

int gitcap_dbg_ffn_txt(const void* X, int ldx, const void* W1pk, const void* W2pk, const float* w1scale, const float* w2scale,
                       const float* b1, int M, int D, int F, float* slabs, void* stream) {
    if (!X || !W1pk || !W2pk || !b1 || !slabs || M <= 0 || !ffn_txt_ok(D, F) || (w1scale != nullptr) != (w2scale != nullptr) || ldx < D ||
        (ldx & 7) || ((uintptr_t)X & 15) || ((uintptr_t)W1pk & 15) || ((uintptr_t)W2pk & 15) || ((uintptr_t)slabs & 15))
        return GITCAP_ERR_ARG;
    FfnTxtArgs a{};
    a.X = (const bf16_t*)X; a.ldx = ldx; a.W1pk = W1pk; a.W2pk = W2pk; a.w1scale = w1scale; a.w2scale = w2scale; a.b1 = b1;
    a.M = M; a.D = D; a.F = F; a.slabs = slabs;
    return dbg_rc(launch_ffn_txt(a, (hipStream_t)stream));
}

// the tables of a variable-length hook (device int32 [n]) on the host: the stream is drained first (the caller may have
// filled them on it)
static bool dbg_read_tables(const int32_t* off, const int32_t* len, int n, hipStream_t s, std::vector<int32_t>& ho, std::vector<int32_t>& hl) {
    if (!off || !len || n <= 0 || ((uintptr_t)off & 3) || ((uintptr_t)len & 3)) return false;
    ho.resize(n); hl.resize(n);
    return hipStreamSynchronize(s) == hipSuccess && hipMemcpy(ho.data(), off, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess &&
           hipMemcpy(hl.data(), len, (size_t)n * 4, hipMemcpyDeviceToHost) == hipSuccess;
}

int gitcap_dbg_attn_full_varlen(const void* qkv, void* ctx, int G, const int32_t* off, const int32_t* len, int H, void* stream) {
    if (!qkv || !ctx || G <= 0 || H <= 0) return GITCAP_ERR_ARG;
    std::vector<int32_t> ho, hl;
    if (!dbg_read_tables(off, len, G, (hipStream_t)stream, ho, hl)) return GITCAP_ERR_ARG;
    int mx = 0;
    for (int g = 0; g < G; ++g) {
        if (ho[g] < 0 || hl[g] < 1) return GITCAP_ERR_ARG;
        mx = std::max(mx, hl[g]);
    }
    return launch_attn_full_varlen((const bf16_t*)qkv, (bf16_t*)ctx, G, off, len, mx, H, (hipStream_t)stream) == hipSuccess ? 0 : GITCAP_ERR_HIP;
}

static int dbg_txt_block(const gitcap_dbg_txt_block_args* g, const int32_t* off, const int32_t* len, void* stream);
int gitcap_dbg_txt_block(const gitcap_dbg_txt_block_args* g, void* stream) { return dbg_txt_block(g, nullptr, nullptr, stream); }
// variable-length form: off / len device int32 [clips], clips = ceil(rows / beams); S_img is not read
int gitcap_dbg_txt_block_varlen(const gitcap_dbg_txt_block_args* g, const int32_t* off, const int32_t* len, void* stream) {
    if (!g || g->rows <= 0 || g->beams <= 0) return GITCAP_ERR_ARG;
    std::vector<int32_t> ho, hl;
    const int clips = (g->rows - 1) / g->beams + 1;
    if (!dbg_read_tables(off, len, clips, (hipStream_t)stream, ho, hl)) return GITCAP_ERR_ARG;
    for (int c = 0; c < clips; ++c)
        if (ho[c] < 0 || hl[c] < 0 || (g->v8_img && (int64_t)ho[c] + hl[c] > g->v8_pitch)) return GITCAP_ERR_ARG;
    return dbg_txt_block(g, off, len, stream);
}

static int dbg_txt_block(const gitcap_dbg_txt_block_args* g, const int32_t* off, const int32_t* len, void* stream) {
    if (!g || !g->kv_img || !g->kv_txt || !g->aow || !g->aob || !g->g1 || !g->b1 || !g->xin || !g->part || !g->cnt || !g->xs || !g->xsb)
        return GITCAP_ERR_ARG;
    if (g->rows <= 0 || g->beams <= 0 || g->T <= 0 || g->t0 < 0 || g->t0 + g->T > g->Tmax || g->S_img < 0 || !txt_block_ok(g->D) ||
        g->H * 64 != g->D || (g->v8_img != nullptr) != (g->vs_img != nullptr) ||
        (g->v8_img && !off && g->v8_pitch < (int64_t)((g->rows - 1) / g->beams + 1) * g->S_img))
        return GITCAP_ERR_ARG;
    // the widest access txt_block_kernel makes on each buffer: 16-byte rows of q / k / v and of the output dense (8 bytes of e4m3 codes),
    // 8 bytes of V codes; everything else -- scales, bias, gamma / beta, residual, part, tickets, xs -- one float or word at a time, xsb
    // one bf16 at a time
    if (((uintptr_t)g->kv_img & 15) || ((uintptr_t)g->kv_txt & 15) || ((uintptr_t)g->aow & 15) || ((uintptr_t)g->aowpk & 15) ||
        ((uintptr_t)g->v8_img & 7) || ((uintptr_t)g->vs_img & 3) || ((uintptr_t)g->aoscale & 3) || ((uintptr_t)g->aob & 3) ||
        ((uintptr_t)g->g1 & 3) || ((uintptr_t)g->b1 & 3) || ((uintptr_t)g->xin & 3) || ((uintptr_t)g->part & 3) || ((uintptr_t)g->cnt & 3) ||
        ((uintptr_t)g->xs & 3) || ((uintptr_t)g->xsb & 1))
        return GITCAP_ERR_ARG;
    TxtBlockArgs a{};
    a.kv_img = (const bf16_t*)g->kv_img; a.kv_txt = (const bf16_t*)g->kv_txt;
    a.rows = g->rows; a.beams = g->beams; a.t0 = g->t0; a.T = g->T; a.Tmax = g->Tmax; a.S_img = g->S_img; a.H = g->H; a.D = g->D;
    a.aow = g->aow; a.aowpk = g->aoscale ? nullptr : g->aowpk; a.aoscale = g->aoscale; a.aob = g->aob; a.g1 = g->g1; a.b1 = g->b1;
    a.xin = g->xin; a.eps = g->eps; a.part = g->part; a.cnt = g->cnt; a.xs = g->xs; a.xsb = (bf16_t*)g->xsb;
    a.v8_img = (const unsigned char*)g->v8_img; a.vs_img = g->vs_img; a.v8_pitch = g->v8_pitch; a.nt_kv = g->nt_kv ? 1 : 0;
    a.off = off; a.len = len;
    return dbg_rc(launch_txt_block(a, (hipStream_t)stream));
}

}  // extern "C"

// ---- staging and layout kernels (tests/test_staging_gpu.py): preproc.hip, the plain row kernels of rowops.hip and the text
// embedding of select.hip.  Each hook is ONE launcher on caller-owned device buffers, no handle, no allocation; what the launcher does not check itself and a wrong
// value of which would index outside a buffer (or fault on a misaligned vector access) is refused here, before any launch
extern "C" {

static bool al(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

int gitcap_dbg_preprocess_patches(const uint8_t* frames_hwc_bgr, int nf, int H, int W, int crop, int p, int Kp, void* patches, void* stream) {
    if (!frames_hwc_bgr || !patches || !al(patches, 2) || Kp <= 0 || (Kp & 1)) return GITCAP_ERR_ARG;
    return dbg_rc(launch_preprocess_patches(frames_hwc_bgr, (bf16_t*)patches, nf, H, W, crop, p, Kp, (hipStream_t)stream));
}

int gitcap_dbg_preprocess_stem(const uint8_t* frames_hwc_bgr, int nf, int H, int W, int crop, void* col, void* stream) {
    if (!frames_hwc_bgr || !col || !al(col, 16)) return GITCAP_ERR_ARG;        // one row = four 16-byte stores
    return dbg_rc(launch_preprocess_stem(frames_hwc_bgr, (bf16_t*)col, nf, H, W, crop, (hipStream_t)stream));
}

// launch_im2col checks nothing but the parity of p.  p % 4 == 0 and img % 4 == 0: 16-byte reads, 8-byte writes, Kp in pieces of 4;
// else (p even): two floats, one 4-byte write, Kp in pieces of 2
int gitcap_dbg_im2col(const float* frames, int nf, int img, int p, int Kp, void* patches, void* stream) {
    if (!frames || !patches || nf <= 0 || img <= 0 || p <= 0 || img % p != 0 || (int64_t)Kp < 3 * (int64_t)p * p) return GITCAP_ERR_ARG;
    const bool v4 = p % 4 == 0 && img % 4 == 0;
    if (v4 ? (Kp % 4 != 0 || !al(frames, 16) || !al(patches, 8)) : (Kp % 2 != 0 || !al(frames, 4) || !al(patches, 4))) return GITCAP_ERR_ARG;
    return dbg_rc(launch_im2col(frames, (bf16_t*)patches, nf, img, p, Kp, (hipStream_t)stream));
}

int gitcap_dbg_cast_bf16(const float* in, void* out, int64_t n, void* stream) {
    if (!in || !out || n <= 0 || !al(in, 16) || !al(out, 8)) return GITCAP_ERR_ARG;
    return dbg_rc(launch_cast_bf16(in, (bf16_t*)out, n, (hipStream_t)stream));
}

int gitcap_dbg_dequant_fp8(const void* w8, const float* scale, void* out, int rows, int K, void* stream) {
    if (!w8 || !scale || !out || !al(w8, 16) || !al(scale, 4) || !al(out, 16)) return GITCAP_ERR_ARG;
    return dbg_rc(launch_dequant_fp8((const unsigned char*)w8, scale, (bf16_t*)out, rows, K, (hipStream_t)stream));
}

// the arrays are host arrays of n entries (n <= 4 is checked before they are read)
int gitcap_dbg_dequant_fp8_batch(int n, const void* const* w8, const float* const* scale, void* const* out, const int32_t* rows,
                                 const int32_t* K, void* stream) {
    if (n <= 0 || n > 4 || !w8 || !scale || !out || !rows || !K) return GITCAP_ERR_ARG;
    DequantBatch b{};
    b.n = n;
    for (int i = 0; i < n; ++i) {
        if (rows[i] <= 0 || K[i] <= 0 || !al(w8[i], 16) || !al(scale[i], 4) || !al(out[i], 16)) return GITCAP_ERR_ARG;
        b.w8[i] = (const unsigned char*)w8[i]; b.scale[i] = scale[i]; b.out[i] = (bf16_t*)out[i]; b.K[i] = K[i];
        b.n16[i] = (int64_t)rows[i] * K[i] / 16;
    }
    return dbg_rc(launch_dequant_fp8_batch(b, (hipStream_t)stream));
}

// launch_embed_text checks nothing
int gitcap_dbg_embed_text(const int64_t* ids, int ld_ids, int rows, int T, int t0, const float* word, const float* pos, const float* gamma,
                          const float* beta, float eps, int D, int vocab, float* xf, void* xb, void* stream) {
    if (!ids || !word || !pos || !gamma || !beta || (!xf && !xb) || rows <= 0 || T <= 0 || ld_ids < T || t0 < 0 || vocab <= 0 || D <= 0 ||
        D > 1024 || (D & 3) || (int64_t)rows * T > 0x7fffffff)
        return GITCAP_ERR_ARG;
    if (!al(ids, 8) || !al(word, 16) || !al(pos, 16) || !al(gamma, 16) || !al(beta, 16) || !al(xf, 16) || !al(xb, 8)) return GITCAP_ERR_ARG;
    return dbg_rc(launch_embed_text(ids, ld_ids, rows, T, t0, word, pos, gamma, beta, eps, D, vocab, xf, (bf16_t*)xb, (hipStream_t)stream));
}

int gitcap_dbg_window_scatter(const float* src, float* ring, int B, int n, int F, int head, int rows_per_frame, int D, void* stream) {
    if (!src || !ring || !al(src, 16) || !al(ring, 16)) return GITCAP_ERR_ARG;
    return dbg_rc(launch_window_scatter(src, ring, B, n, F, head, rows_per_frame, D, (hipStream_t)stream));
}

int gitcap_dbg_window_assemble(const float* ring, const float* temporal, void* out, float* vis, int B, int F, int head, int N, int D,
                               void* stream) {
    if (!ring || !out || !al(ring, 16) || !al(temporal, 16) || !al(out, 8) || !al(vis, 16) || (int64_t)B * F * N > 0x7fffffff) return GITCAP_ERR_ARG;
    return dbg_rc(launch_window_assemble(ring, temporal, (bf16_t*)out, vis, B, F, head, N, D, (hipStream_t)stream));
}

// counts: HOST int32 [B], copied into the RaggedCounts the launch takes by value; pos_cap = the entries pos holds
int gitcap_dbg_ragged_tables(const int32_t* counts, int B, int N, int32_t* off, int32_t* len, int32_t* pos, int pos_cap, void* stream) {
    if (!counts || B <= 0 || B > 256 || N <= 0 || !off || !len || !pos || !al(off, 4) || !al(len, 4) || !al(pos, 4)) return GITCAP_ERR_ARG;
    RaggedCounts rc{};
    rc.B = B;
    int64_t total = 0;
    for (int b = 0; b < B; ++b) {
        if (counts[b] < 1 || counts[b] > 255) return GITCAP_ERR_ARG;
        rc.n[b] = (unsigned char)counts[b];
        total += counts[b];
    }
    if (total > pos_cap || total * N > 0x7fffffff) return GITCAP_ERR_ARG;
    return dbg_rc(launch_ragged_tables(rc, N, off, len, pos, (hipStream_t)stream));
}

// pos (device int32 [frames]) is read back first (the call synchronises `stream`): an entry outside [0, temporal_rows) is refused
int gitcap_dbg_ragged_temporal(const float* ln, const float* temporal, int temporal_rows, const int32_t* pos, void* out, float* vis,
                               int frames, int N, int D, void* stream) {
    if (!ln || !temporal || !pos || !out || frames <= 0 || N <= 0 || temporal_rows <= 0 || (int64_t)frames * N > 0x7fffffff || !al(ln, 16) ||
        !al(temporal, 16) || !al(pos, 4) || !al(out, 8) || !al(vis, 16))
        return GITCAP_ERR_ARG;
    std::vector<int32_t> hp((size_t)frames);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess || hipMemcpy(hp.data(), pos, (size_t)frames * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return GITCAP_ERR_HIP;
    for (int f = 0; f < frames; ++f)
        if (hp[f] < 0 || hp[f] >= temporal_rows) return GITCAP_ERR_ARG;
    return dbg_rc(launch_ragged_temporal(ln, temporal, pos, (bf16_t*)out, vis, frames, N, D, (hipStream_t)stream));
}

// the stream pool's host plan on cursors given as heads / counts (touches no device; a refused plan writes nothing)
int gitcap_dbg_pool_plan(int n_streams, int F, int32_t* heads, int32_t* counts, const int32_t* push_ids, int n_push, int32_t* dst,
                         const int32_t* cap_ids, int B, int32_t* src, int32_t* pos, int32_t* off, int32_t* len, int32_t* out3) {
    if (n_streams < 1 || n_streams > 4096 || F < 1 || F > 255 || !heads || !counts || n_push < 0 || B < 0 || n_push > (1 << 20) || B > n_streams ||
        (n_push > 0 && (!push_ids || !dst)) || (B > 0 && (!cap_ids || !src || !pos || !off || !len)) || !out3)
        return GITCAP_ERR_ARG;
    std::vector<RingCursor> cur((size_t)n_streams);
    for (int i = 0; i < n_streams; ++i) {
        if (heads[i] < 0 || heads[i] >= F || counts[i] < 0 || counts[i] > F) return GITCAP_ERR_ARG;
        cur[(size_t)i].slots = F; cur[(size_t)i].head = heads[i]; cur[(size_t)i].count = counts[i];
    }
    std::vector<int32_t> d((size_t)n_push), sp((size_t)B * F * 2), ol((size_t)B * 2);
    PoolPlan plan;
    int bad = -1;
    const int why = pool_plan(cur, push_ids, n_push, d.data(), cap_ids, B, sp.data(), sp.data() + (size_t)B * F, ol.data(), ol.data() + B, &plan, &bad);
    if (why) return why == POOL_PLAN_EMPTY ? GITCAP_ERR_STATE : GITCAP_ERR_ARG;
    for (int i = 0; i < n_streams; ++i) { heads[i] = cur[(size_t)i].head; counts[i] = cur[(size_t)i].count; }
    for (int i = 0; i < n_push; ++i) dst[i] = d[(size_t)i];
    for (int g = 0; g < plan.total; ++g) { src[g] = sp[(size_t)g]; pos[g] = sp[(size_t)B * F + g]; }
    for (int r = 0; r < B; ++r) { off[r] = ol[(size_t)r]; len[r] = ol[(size_t)B + r]; }
    out3[0] = plan.total; out3[1] = plan.maxn; out3[2] = plan.dense ? 1 : 0;
    return 0;
}

// a device int32 table read back (the call synchronises `stream`): false when it cannot be read or an entry is outside [0, limit)
static bool dbg_table_ok(const int32_t* tab, int n, int limit, void* stream, std::vector<int32_t>& host, int* rc) {
    host.resize((size_t)n);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess || hipMemcpy(host.data(), tab, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) {
        *rc = GITCAP_ERR_HIP;
        return false;
    }
    *rc = GITCAP_ERR_ARG;
    for (int i = 0; i < n; ++i)
        if (host[(size_t)i] < 0 || host[(size_t)i] >= limit) return false;
    return true;
}

int gitcap_dbg_pool_scatter(const float* stage, float* ring, int ring_frames, const int32_t* dst, int frames, int N, int D, void* stream) {
    if (!stage || !ring || !dst || ring_frames <= 0 || frames <= 0 || frames > ring_frames || !al(stage, 16) || !al(ring, 16) || !al(dst, 4))
        return GITCAP_ERR_ARG;
    std::vector<int32_t> hd;
    int rc = 0;
    if (!dbg_table_ok(dst, frames, ring_frames, stream, hd, &rc)) return rc;
    std::vector<char> seen((size_t)ring_frames, 0);
    for (int32_t d : hd)
        if (seen[(size_t)d]++) return GITCAP_ERR_ARG;        // one writer per ring frame
    return dbg_rc(launch_pool_scatter(PoolScatterArgs{stage, ring, dst, frames, N, D}, (hipStream_t)stream));
}

int gitcap_dbg_pool_assemble(const float* ring, int ring_frames, const float* temporal, int temporal_rows, const int32_t* src,
                             const int32_t* pos, void* out, int frames, int N, int D, void* stream) {
    if (!ring || !src || !out || ring_frames <= 0 || frames <= 0 || (temporal && (!pos || temporal_rows <= 0)) || !al(ring, 16) ||
        !al(temporal, 16) || !al(src, 4) || !al(pos, 4) || !al(out, 8))
        return GITCAP_ERR_ARG;
    std::vector<int32_t> ht;
    int rc = 0;
    if (!dbg_table_ok(src, frames, ring_frames, stream, ht, &rc)) return rc;
    if (temporal && !dbg_table_ok(pos, frames, temporal_rows, stream, ht, &rc)) return rc;
    return dbg_rc(launch_pool_assemble(PoolAssembleArgs{ring, temporal, src, pos, (bf16_t*)out, frames, N, D}, (hipStream_t)stream));
}

// the entry strides are in floats; rows are copied 16 bytes at a time
int gitcap_dbg_gather_hidden(const float* img, const float* txt, float* out, int n_entries, int B, int S_img, int T, int D,
                             int64_t img_entry_stride, int64_t txt_entry_stride, void* stream) {
    if (!img || !txt || !out || !al(img, 16) || !al(txt, 16) || !al(out, 16) || img_entry_stride < 0 || txt_entry_stride < 0 ||
        (img_entry_stride & 3) || (txt_entry_stride & 3))
        return GITCAP_ERR_ARG;
    return dbg_rc(launch_gather_hidden(img, txt, out, n_entries, B, S_img, T, D, (size_t)img_entry_stride, (size_t)txt_entry_stride,
                                       (hipStream_t)stream));
}

// gather_txt_rows_kernel copies a row's first t_len positions as t_len * width / 8 pieces of 16 bytes (8 bf16), from row bases at
// multiples of Tmax * width behind layer bases at multiples of layer_stride: all three must be multiples of 8 elements.  src_rows
// (device int32 [rows]) is read back first (the call synchronises `stream`): src and dst hold `rows` rows per layer
int gitcap_dbg_gather_txt_rows(const void* src, void* dst, const int32_t* src_rows, int rows, int t_len, int Tmax, int width, int layers,
                               int64_t layer_stride, void* stream) {
    if (!src || !dst || src == dst || !src_rows || rows <= 0 || layers <= 0 || width <= 0 || Tmax <= 0 || t_len < 0 || t_len > Tmax ||
        !al(src, 16) || !al(dst, 16) || !al(src_rows, 4))
        return GITCAP_ERR_ARG;
    const int64_t row = (int64_t)Tmax * width;
    if (row > 0x7fffffff || (((int64_t)t_len * width) & 7) || (row & 7) || (layer_stride & 7) || layer_stride < (int64_t)rows * row) return GITCAP_ERR_ARG;
    std::vector<int32_t> hr((size_t)rows);
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess || hipMemcpy(hr.data(), src_rows, (size_t)rows * 4, hipMemcpyDeviceToHost) != hipSuccess)
        return GITCAP_ERR_HIP;
    for (int r = 0; r < rows; ++r)
        if (hr[r] < 0 || hr[r] >= rows) return GITCAP_ERR_ARG;
    return dbg_rc(launch_gather_txt_rows((const bf16_t*)src, (bf16_t*)dst, src_rows, rows, t_len, Tmax, width, layers, (size_t)layer_stride,
                                         (hipStream_t)stream));
}

}  // extern "C"
