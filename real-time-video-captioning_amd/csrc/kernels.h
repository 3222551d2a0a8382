// Launcher declarations for the gfx950 kernels behind libgitcap's C ABI.
#pragma once
#include "common.h"
#include "host_logic.h"      // PromptArgs, RaggedCounts: the plain option structs that travel to kernels by value
#include <atomic>
#include <cstddef>

// ---- big-tile bf16 MFMA GEMM:  C[m][n] = sum_k A[m][k] * W[n][k]  (+ epilogue) (gemm.hip, gemm256.hip) ----
enum GemmEpi {
    EPI_BIAS_BF16 = 0,        // out bf16 = acc + bias
    EPI_BIAS_QGELU_BF16 = 1,  // out bf16 = quick_gelu(acc + bias)      (CLIP MLP)
    EPI_BIAS_GELU_BF16 = 2,   // out bf16 = erf_gelu(acc + bias)        (BERT intermediate)
    EPI_BIAS_RESID_F32 = 3,   // out f32  = acc + bias + resid          (out may alias resid)
    EPI_BIAS_F32 = 4,         // out f32  = acc + bias
    EPI_PATCH_F32 = 5,        // out f32 row (frame*N + 1 + patch) = acc + pos[1+patch]
    // 256x256 kernel only, N = 768 or 1024: the tiles of one row block exchange LayerNorm statistics (ln_canon.h)
    // and each normalises its own columns -> the LayerNorm launch behind the GEMM and its re-read disappear.
    EPI_RESID_LN_PRE = 6,     // x = acc + bias + resid: out f32 = x (nullable), ln_out bf16 = LayerNorm(x) [+ ln_add] (pre-LN ViT block; ln_post)
    EPI_RESID_LN_POST = 7,    // x = acc + bias [+ resid]: out f32 = LayerNorm(x), ln_out bf16 = the same (post-LN decoder)
    // fp8 kernel only (gemm256.hip: gemm256f8_kernel): the GELU output as OCP e4m3 codes of y * out8_inv -- the activation operand of the next fp8 GEMM
    EPI_BIAS_QGELU_F8 = 8,    // out e4m3 = quick_gelu(acc + bias)
    EPI_BIAS_GELU_F8 = 9      // out e4m3 = erf_gelu(acc + bias)
};
struct GemmArgs {
    const bf16_t* A; int lda;     // activations [M][lda], M multiple of 128 (padded rows are junk)
    const bf16_t* W;              // weights [N][K] (torch Linear layout), N multiple of 128
    const float* bias;            // [N] or nullptr
    int M, N, K;                  // K multiple of 64
    void* out; int ldo;
    const float* resid; int ldr;
    const float* pos;             // EPI_PATCH: [tokens_per_frame][N]
    int tokens_per_frame, patches_per_frame, valid_rows;
    // EPI_RESID_LN_*: LayerNorm of the output rows
    const float *ln_g, *ln_b; float ln_eps;
    bf16_t* ln_out; int ld_ln;    // bf16 LayerNorm output
    const float* ln_add;          // nullable (PRE): LayerNorm output += ln_add[((row / ln_add_div) % ln_add_mod) * N + n]  (temporal embedding)
    int ln_add_div, ln_add_mod;
    float* ln_out_f32; int ld_ln_f32;   // nullable (PRE): fp32 copy of the LayerNorm output, rows < valid_rows only (caller's unpadded buffer)
    float2* ln_stats;             // [ln_stats_rows][16] per-segment (mean, M2) exchanged between the tiles of a row block
    unsigned* ln_cnt;             // [row blocks][2] per row block {arrivals, generation}: zero before the first launch, self-resetting
    int ln_stats_rows;            // rows of ln_stats (>= M)
    int ln_rowblock_map;          // set by the launcher: workgroup -> tile map hands every XCD whole row blocks (host_logic.h)
    // fp8 compute (gemm256.hip: gemm256f8_kernel): A and W point at e4m3 codes; the accumulators are multiplied by ascale * wscale[n]
    const float* wscale; float ascale;
    float out8_inv;               // EPI_BIAS_*GELU_F8: 1 / (static scale of the e4m3 output)
    unsigned char* ln_out8; int ld_ln8; float ln_out8_inv;   // nullable (EPI_RESID_LN_*): e4m3 copy of the LayerNorm output * ln_out8_inv
    unsigned* ln_fail;            // nullable: host-visible word raised when a tile gave up waiting for its siblings (no trap)
    unsigned ln_spin_limit;       // polls (~0.3 us each) before giving up; 0 = the default (~30 s)
    unsigned long long* f8_sat;   // nullable: device counter of e4m3 activation codes (valid rows) the epilogue clamped at +-448
                                  // (LAST: the residual + LayerNorm epilogue runs at the 256-VGPR limit and where the compiler spills
                                  // depends on the kernarg layout -- tests/test_isa_lint.py: test_gemm_ln_epilogue_keeps_its_spills_out_of_the_row_loops)
};
static_assert(offsetof(GemmArgs, f8_sat) + sizeof(unsigned long long*) == sizeof(GemmArgs), "f8_sat must stay the LAST field of GemmArgs (see its comment)");
constexpr unsigned LN_SPIN_DEFAULT = 1u << 26;
int device_cus();                 // compute units of the current device (cached per device; 256 when the query fails)
hipError_t launch_gemm(const GemmArgs& a, int epi, hipStream_t s);      // 128x128 tile (any M%128, N%128)
hipError_t launch_gemm64(const GemmArgs& a, int epi, hipStream_t s);    // 64x64 tile, 3-stage ring (few-hundred-row launches)
bool gemm256_ok(const GemmArgs& a);
hipError_t launch_gemm256(const GemmArgs& a, int epi, hipStream_t s);   // 256x256 tile, 8-wave ping-pong
bool gemm256_ln_ok(const GemmArgs& a);                                   // shape the EPI_RESID_LN_* epilogues accept
bool gemm256f8_ok(const GemmArgs& a);                                    // fp8 operands: K % 128 == 0, wscale / ascale set
hipError_t launch_gemm256f8(const GemmArgs& a, int epi, hipStream_t s);  // the same tile kernel on e4m3 operands (gemm256.hip)

// ---- skinny GEMMs (text rows; M = a few 16-row tiles): weight streaming, one wave per tile (skinny.hip) ----
enum SkinnyEpi { SK_BIAS_BF16 = 0, SK_BIAS_GELU_BF16 = 1, SK_BIAS_RELU_BF16 = 2, SK_BIAS_F32 = 3 };
struct SkinnyArgs {
    const bf16_t* X; int ldx;     // bf16 activations, row m at X + m*ldx
    const void* W;                // [Npad16][K] bf16, or e4m3 bytes when wscale != nullptr
    const float* wscale;          // nullable: [Npad16] per-row power-of-two scale of e4m3 weights
    const float* bias;            // [N] (full kernel only)
    int M, N, K;                  // M valid rows, N valid cols (weight rows padded to 16)
    void* out;                    // full: row m -> out + orow(m)*ldo, orow(m) = (m / T)*row_stride + row_off + m % T
    int ldo, T, row_stride, row_off;   // splitk: out = fp32 slabs [ksplit][M][ldo]
    float* amax_val; int* amax_idx;    // SK_BIAS_F32 only (nullable): per-tile arg-max partials [M][ntiles]
    // Optional row prologue (kind != 0; M <= 2, K = the row width, bf16 weights): every workgroup computes the M input rows
    // itself -- the LayerNorm that would otherwise be the launch in front of this one -- while its weight fragments are
    // in flight; X is not read.  Workgroup 0 also writes the fp32 rows to xf (must not alias resid).
    struct RowPrologue {
        int kind;                          // 0 none, 1 split-K slabs + bias + residual -> LayerNorm, 2 text embedding -> LayerNorm
        const float* slabs; int nslab;     // kind 1
        const float *bias, *resid;
        const int64_t* ids;                // kind 2
        int ld_ids, T, t0, vocab;
        const float *word, *pos;
        const float *g, *b; float eps;     // LayerNorm
        float* xf;                         // [M][K]
    } ln;
    // optional fragment-major copy of W (launch_pack_frags: [tile][k32][lane][8]); when set the kernels read it instead of W
    const void* Wpk;
    int ksplit;                            // splitk: number of K slabs (0: skinny_ksplit(K))
    // SK_BIAS_F32 with amax_val set (nullable): third per-tile partial [M][ntiles], sum of exp(logit - amax_val) over the tile's
    // valid columns (0 where amax_val is -inf) -- what launch_argmax_final / launch_draft_accept turn into the chosen token's
    // log-probability.  nullptr: the launch is the one without it.
    float* amax_sum;
};
extern std::atomic<bool> g_row_prologue;                                 // gitcap.hip: GITCAP_NO_ROW_PROLOGUE / gitcap_dbg_config(1, .)
// vocabulary head: four 16-column tiles per workgroup share the activation rows through LDS (skinny.hip: skinny_head_kernel);
// GITCAP_NO_HEAD_SHARE / gitcap_dbg_config(10, 0): one single-wave workgroup per tile.  Same bits either way.
extern std::atomic<bool> g_head_share;
// gitcap.hip, gitcap_dbg_config(20, .): a prompted greedy loop of either handle runs the positions every row's prompt covers as one pass
extern std::atomic<bool> g_prompt_prefill;
// one/two-row prologue over more than 16 slabs: three-wave workgroups that share the reduce (skinny.hip: skinny_rows3_kernel);
// GITCAP_NO_ROWS3 / gitcap_dbg_config(11, 0): the single-wave form.  Same bits either way.
extern std::atomic<bool> g_rows3;
bool skinny_row_prologue_ok(int M, int K, bool fp8);         // shapes the row-prologue form is instantiated for
// Target capture of the scoring head (gitcap_score; kernels of their own, skinny.hip "LSE plus target"): head row m is position
// j = m % T of id row m / T and its target is ids[(m / T) * ld + j + shift] -- none when j + shift >= T.  The lane that holds that
// column of row m also stores the fp32 logit to logit[m]; a target outside [0, N) stores nothing.
struct HeadTargets { const int64_t* ids; int T, ld, shift; float* logit; };
// Ban mask of the constrained vocabulary head (gitcap_attach_constraints; kernels of their own, skinny.hip "BAN"): uint16
// [rows][ld], bit c & 15 of word c >> 4 of row m set = column c of head row m is banned; one word = one 16-column tile.
// ld >= ceil(N / 16) and even (rows 4-byte aligned).  A banned column's logit is -inf before a.out, the arg-max partial and
// the sum partial are formed.  Built by launch_ban_mask / launch_ban_mask_rec (search.hip).
struct HeadBan { const uint16_t* mask; int ld; };
// tg (nullable): SK_BIAS_F32 with all three partial buffers set; a.out stays nullable
// bn (nullable; not with tg or a row prologue): SK_BIAS_F32, the BAN form of the head (plain, or with amax_sum the LSE form)
hipError_t launch_skinny(const SkinnyArgs& a, int epi, hipStream_t s, const HeadTargets* tg = nullptr, const HeadBan* bn = nullptr);
// The vocabulary head's launch_skinny(SK_BIAS_F32) arguments over the bf16 rows xb [rows * T][D] (host only): every position
// (all_positions) or the last position of every row.  The partial buffers are nullable.  Returns the row stride and offset at
// which launch_argmax_final finds the last position of each row among the head's rows.
struct HeadWeight { const void *W, *Wpk; const float *wscale, *bias; int V, D; };    // row-major, optional fragment-major copy / row scales
struct HeadRows { int am_stride, am_off; };
inline HeadRows vocab_head_args(SkinnyArgs& ha, const HeadWeight& hw, const bf16_t* xb, int rows, int T, bool all_positions,
                                float* logits_out, float* amax_val, int* amax_idx, float* amax_sum) {
    ha = SkinnyArgs{};
    ha.W = hw.W; ha.Wpk = hw.Wpk; ha.wscale = hw.wscale; ha.bias = hw.bias; ha.N = hw.V; ha.K = hw.D; ha.ldo = hw.V;
    ha.T = 1; ha.row_stride = 1; ha.row_off = 0; ha.out = logits_out;
    ha.amax_val = amax_val; ha.amax_idx = amax_idx; ha.amax_sum = amax_sum;
    HeadRows r{1, 0};
    if (all_positions) {
        ha.X = xb; ha.ldx = hw.D; ha.M = rows * T;
        r.am_stride = T; r.am_off = T - 1;
    } else {
        ha.X = xb + (size_t)(T - 1) * hw.D; ha.ldx = T * hw.D; ha.M = rows;
    }
    return r;
}
// ---- top-k alternatives of a head row (gitcap_attach_top_logprobs; skinny.hip: head_topk_kernel) --------------------------------
// Columns are ordered by (logit descending, column ascending), launch_argmax_final's tie rule.  A tile's arg-max partial is its
// best column under that order, the representatives of different tiles are different columns, and a column among the row's k best
// has its tile's representative ahead of it: the k best columns lie in the k best tiles by (val, idx).  One workgroup per output
// row picks those tiles from the row's partials, recomputes their 16 logits each with the head's own MFMA chain over the head's
// operands (the head's bits; bias added, banned columns -inf, columns >= V no candidates) and ranks the candidates:
//     top_ids[j] = the j-th best column, top_lp[j] = (logit - M) - log(z), M and z the row's maximum and merged sum as
//     lp_partials forms them: rank 0 is launch_argmax_final's token and compares == to its log-probability.
// Ranks the row cannot fill (fewer than k columns above -inf) hold id -1 and lp -inf.  1 <= k <= HEAD_TOPK_MAX.
// Output row i < rows * T reads head row m = (i / T) * row_stride + row_off + i % T (X + m * ldx, partials and mask row m) and
// writes k entries at ((i / T) * ld + i % T) * k: T = 1 with launch_argmax_final's row map for a token step, T = positions - 1
// and row_stride = positions for a scoring pass.  A row's output does not depend on the rows beside it.
// run_head: the launcher first runs the LSE head (with bn its BAN form) over the M head rows into val / idx / sum.
constexpr int HEAD_TOPK_MAX = 32;
struct HeadTopkArgs {
    const bf16_t* X; int ldx;
    HeadWeight hw;
    float* val; int* idx; float* sum;       // [head rows][ceil(V / 16)]
    const HeadBan* bn;                      // nullable: the mask the head ran under (head row m = mask row m)
    bool run_head; int M;                   // run_head: the head rows of the launch
    int rows, T, row_stride, row_off;
    int k; int64_t* top_ids; float* top_lp; int ld;
};
bool head_topk_ok(int D, bool fp8);                          // widths the kernel is instantiated for (launch_skinny's)
hipError_t launch_head_topk(const HeadTopkArgs& a, hipStream_t s);
// ---- teacher-student divergence (gitcap_distill): both vocabulary heads over the same tiles, then one merge -------------------
// launch_head_dual (skinny.hip: skinny_head_dual_kernel): the teacher's rows Xt [M][ldxt] against wt (bf16, or e4m3 codes with
// wscale) and the student's rows Xs [M][ldxs] against ws (bf16), (wt.D, ws.D) one of (768, 576), (1024, 576), (128, 64), equal V.
// With t = (acc + bias) * inv_temp and s likewise it leaves seven partials [M][ntiles]: each model's arg-max / sum-of-exp partials
// as the single heads leave them (inv_temp == 1: bit for bit) and cross = sum exp(t - t_max) ((t - t_max) - (s - s_max)) over the
// tile's columns with t > -inf (+inf where such a column has s = -inf, 0 where t_max = -inf).  tg.ids (nullable): the logits t / s
// of each head row's target column go to tg.logit / s_logit (HeadTargets; untouched for a target outside [0, V)).
struct DualHeadArgs {
    const bf16_t *Xt, *Xs; int ldxt, ldxs;
    HeadWeight wt, ws;
    int M; float inv_temp;
    float *t_max; int* t_idx; float *t_sum, *s_max; int* s_idx; float *s_sum, *cross;
    HeadTargets tg; float* s_logit;
};
bool head_dual_ok(int Kt, int Ks);
hipError_t launch_head_dual(const DualHeadArgs& a, hipStream_t s);
bool skinny_full_ok(int K);                                 // K depths launch_skinny is instantiated for
int skinny_ksplit(int K);                                    // number of K slabs launch_skinny_splitk writes
hipError_t launch_skinny_splitk(const SkinnyArgs& a, hipStream_t s);

// ---- fused FC1 -> GELU -> FC2 of the text rows over hidden slices (ffn_txt.hip) -----------------------------------------
// Workgroup s owns hidden units 64 s .. 64 s + 63: h = GELU(X W1_s^T + b1_s) rounded to bf16 (exactly the FC1 launch's
// output), then its split-K share of FC2, slab[s][m][:] = h W2[:, slice]^T (fp32).  The slabs are summed by
// launch_ln_reduce / the row prologue (nslab = F / 64).  Bitwise equal to launch_skinny (FC1 + GELU) followed by
// launch_skinny_splitk with ksplit = F / 64.
struct FfnTxtArgs {
    const bf16_t* X; int ldx;                   // [M][D] bf16
    const void *W1pk, *W2pk;                    // fragment-major FC1 [F][D] / FC2 [D][F]: bf16, or e4m3 codes when w1scale != nullptr
    const float *w1scale, *w2scale;             // nullable: per-row power-of-two scales of e4m3 weights ([F] / [D])
    const float* b1;                            // [F]
    int M, D, F;
    float* slabs;                               // [F / 64][M][D]
};
bool ffn_txt_ok(int D, int F);
hipError_t launch_ffn_txt(const FfnTxtArgs& a, hipStream_t s);
// ---- the text rows' kernels around the decoder stack (select.hip) ------------------------------------------------------------------
// token selection: host-only records, passed by const&; the kernels receive their scalars and pointers
// emb (nullable; greedy loop, one position per row): the kernel goes on to embed the token it just chose at text position
// emb->position -- word + position embedding -> LayerNorm -> xf / xb row r (rowln.h: the code of launch_embed_text) -- so
// the next token step starts at its q|k|v projection.
struct NextEmbed { const float *word, *pos, *gamma, *beta; float eps; int D, vocab, position; float* xf; bf16_t* xb; };
struct ArgmaxArgs {
    // the head's per-tile partials [head rows][ntiles] (SkinnyArgs::amax_val / amax_idx / amax_sum of the same head launch)
    const float* val; const int* idx;
    const float* sum;             // nullable, with lp_out (both or neither)
    int ntiles;
    // out[r*ld_out] = index of the max over the per-tile partials of row r*row_stride + row_off, r < rows; lowest index wins ties
    // (torch.argmax on CPU), 0 when the winner is an empty tile's index 0x7fffffff (no logit above -inf in the row)
    int rows, row_stride, row_off;
    int64_t* out; int ld_out;
    int32_t* sep_cnt; int step, sep_id;   // sep_cnt != nullptr: sep_cnt[step] += 1 for every row whose token is sep_id (zero it per call)
    // lp_out[r*ld_lp] = log_softmax(logits)[token] of row r, natural log, -inf for a row with no logit above -inf.  Fixed summation
    // order: bitwise independent of `rows`.
    float* lp_out; int ld_lp;
    const NextEmbed* emb;         // nullable (above)
    // prompt (PromptArgs, host_logic.h; nullable) + prompt_pos = the position the launch writes: a row with prompt_pos < lengths[r]
    // takes ids[r][prompt_pos] instead of its arg-max (out, the embedded next row), leaves sep_cnt alone and gets lp 0.0f; with
    // prompt_pos >= max_len the launch is the one without a prompt.
    const PromptArgs* prompt; int prompt_pos;
    // keep_len (nullable, device int32 [rows]; not with a prompt): the KEEP form -- a row with prompt_pos < keep_len[r] keeps
    // out[r] and lp_out[r] as they stand, leaves sep_cnt alone and embeds its next row from the id already in out[r]
    // (launch_draft_accept_rows wrote them); every other row is the plain launch's.
    const int32_t* keep_len;
};
hipError_t launch_argmax_final(const ArgmaxArgs& a, hipStream_t s);
// text embedding + LN: row m=(r, j) -> token ids[r*ld_ids + j], position t0 + j
hipError_t launch_embed_text(const int64_t* ids, int ld_ids, int rows, int T, int t0,
                             const float* word, const float* pos, const float* gamma, const float* beta,
                             float eps, int D, int vocab, float* x_f32, bf16_t* x_bf16, hipStream_t s);
// x = LayerNorm(sum_s slab[s][m][:] + bias + resid[m][:]) -> xf (fp32) and xb (bf16); one wave per row
hipError_t launch_ln_reduce(const float* slabs, int nslab, const float* bias, const float* resid,
                            const float* gamma, const float* beta, float eps, int M, int D,
                            float* xf, bf16_t* xb, hipStream_t s);
// Draft verification of the student's greedy loop: the partials hold B x n rows (row r * n + j = position j of caption r, n <= 63);
// reduces them under launch_argmax_final's tie rule and compares with the draft tokens staged in ids [B][ld] (columns 1..n; -1 =
// not a word).  a = the leading positions at which every row's token equals its draft token; ids columns 1..min(a + 1, n) and
// sep_cnt[0 .. min(a + 1, n) - 1] become what the token loop would have written; host = {a, all rows emitted SEP in one of those steps}.
struct DraftAcceptArgs {
    const float* val; const int* idx;
    const float* sum;             // nullable, with lp_out (both or neither)
    int ntiles, B, n;
    int64_t* ids; int ld;
    int* tok;                     // int[B * n] scratch
    unsigned* ticket;             // one word, zero between launches
    int32_t* sep_cnt; int sep_id;
    int32_t* host;                // page-locked int32[2]
    // lp_out[r*ld_lp + j] = the log-probability of the token at position j (launch_argmax_final's value of that row) for the covered
    // positions; columns behind them are not written.  lp_tok: int[B * n] scratch, ld_lp >= n.
    int* lp_tok; float* lp_out; int ld_lp;
};
hipError_t launch_draft_accept(const DraftAcceptArgs& a, hipStream_t s);
// Draft verification of the teacher's greedy loop, accepted row by row.  launch_draft_stage: ids [rows][ld] column 0 = cls, columns
// 1..n = draft [rows][ld_draft] columns 1..n, an id outside [0, vocab) as -1.  launch_draft_accept_rows: launch_draft_accept's
// partials and tie rule, but per caption r: a_r = its leading matching positions, covered_r = min(a_r + 1, n); ids[r][1..covered_r],
// len[r] = 1 + covered_r (ArgmaxArgs::keep_len), lp_out[r*ld_lp + j] for j < covered_r, sep_cnt[j] += 1 per covered SEP (atomic: the
// caller zeroes sep_cnt), host_rows[r] = a_r; host = {min covered, max covered, sum of a_r, some j < min covered has sep_cnt[j] == B}.
// Nothing behind a caption's covered part is written.
struct DraftAcceptRowsArgs {
    const float* val; const int* idx;
    const float* sum;             // nullable, with lp_out (both or neither)
    int ntiles, B, n;             // n <= 63
    int64_t* ids; int ld;
    int32_t* len;                 // device int32[B]
    int* tok;                     // int[B * n] scratch
    int* row_res;                 // int[2 * B] scratch
    unsigned* ticket;             // 1 + B words, zero between launches
    int32_t* sep_cnt; int sep_id;
    int32_t* host;                // page-locked int32[4]
    int32_t* host_rows;           // nullable: page-locked int32[B]
    int* lp_tok; float* lp_out; int ld_lp;      // lp_tok: int[B * n] scratch, ld_lp >= n
};
hipError_t launch_draft_stage(const int64_t* draft, int ld_draft, int n, int rows, int vocab, int64_t cls, int64_t* ids, int ld, hipStream_t s);
hipError_t launch_draft_accept_rows(const DraftAcceptRowsArgs& a, hipStream_t s);
// Teacher-forced scoring of given captions ids [rows][ld_ids] (CLS first) from the head's partials of all rows x T positions
// (row m = r * T + j) and the target logits the scoring head captured (HeadTargets with shift 1).  Position (r, j), j < T - 1,
// is counted unless its target y = ids[r][j + 1] lies outside [0, V), equals ignore_id, or lengths (nullable, device) has
// j + 1 >= lengths[r].  One workgroup per (r, j): top1_ids / top1_lp [rows][T - 1] (nullable) = launch_argmax_final's token and
// log-probability of row m, bit for bit; lp[r * ld_lp + j] = (logit[m] - max) - log(total) of a counted position (-inf for a
// -inf target logit, never NaN), 0 of an ignored one.  row_sum / row_cnt (nullable; a second launch, one thread per row) = the
// sum of the counted positions' lp in ascending position order and their number.  lp is required (the caller's or a scratch).
struct ScoreOut { float* lp; int ld_lp; float* row_sum; int32_t* row_cnt; int64_t* top1_ids; float* top1_lp; };
hipError_t launch_score_final(const float* amax_val, const int* amax_idx, const float* amax_sum, int ntiles, const float* tgt_logit,
                              const int64_t* ids, int ld_ids, int rows, int T, const int32_t* lengths, int64_t ignore_id, int V,
                              const ScoreOut& o, hipStream_t s);
// launch_distill_final (select.hip): one workgroup per (row r, position j < T) merges the partials of head row m = r * T + j in
// launch_score_final's fixed order: each model's winner and log-sum-exp exactly as score_final_kernel forms them, C = sum over the
// tiles of e^(t_max - Mt) (cross + t_sum ((t_max - Mt) - (s_max - Ms))), kl = C / Zt - log Zt + log Zs (a value in [-DISTILL_CLAMP,
// 0) becomes 0, DISTILL_CLAMP = the two logs' share of the rounding bound: tests/distill_reference.py; +inf where the teacher puts mass on a column the
// student excludes; 0 for a row the teacher gives no column at all).  A position j >= lengths[r] (nullable) gets kl 0 and is not
// counted.  top1 / agree [rows][T] cover every position; t_lp / s_lp [rows][ld_lp] = the given next token's log-probability at
// positions 0 .. T - 2 under launch_score_final's rules (0 where ignored), need t_logit / s_logit.  All outputs but kl nullable.
// row_kl_sum / row_cnt (a second launch, one thread per row): the counted positions' kl in ascending order, and their number.
constexpr float DISTILL_CLAMP = 4e-5f;                     // 2 x the 2e-5 nats of a merged log-sum-exp
struct DistillOut {
    float* kl; int ld_kl; int64_t *t_top1, *s_top1; uint8_t* agree; float *t_lp, *s_lp; int ld_lp; float* row_kl_sum; int32_t* row_cnt;
};
struct DistillPartials { const float* t_max; const int* t_idx; const float *t_sum, *s_max; const int* s_idx; const float *s_sum, *cross; };
hipError_t launch_distill_final(const DistillPartials& p, int ntiles, const float* t_logit, const float* s_logit, const int64_t* ids,
                                int ld_ids, int rows, int T, const int32_t* lengths, int64_t ignore_id, int V, const DistillOut& o,
                                hipStream_t s);
hipError_t launch_finish_steps(const int32_t* sep_cnt, int rows, int max_len, int stop, int32_t* steps_out, hipStream_t s);
hipError_t launch_fill_i64(int64_t* p, int ld, int rows, int64_t v, hipStream_t s);
// p[r][0 .. lengths[r] - 1] = prompt.ids[r][the same], r < rows (ld >= prompt.max_len): the start of a prompted greedy loop
hipError_t launch_fill_prompt(int64_t* p, int ld, int rows, const PromptArgs& prompt, hipStream_t s);
// ---- host-only composites of the launchers above, defined here -----------------------------------------------------------------
// The scoring head over the bf16 rows xb [rows * T][D] + launch_score_final (host only; what gitcap_score / gitcap_student_score
// run behind their decoder stacks).  scratch: fp32 [2][rows * T] = the target logits, then the lp rows where the caller wants none.
// topk (k != 0; gitcap_attach_top_logprobs): also the k best columns of positions 0 .. T - 2 of every row, counted or not, to
// topk.ids / topk.lp [rows][topk.ld][k] (launch_head_topk over the same partials: rank 0 = top1_ids / top1_lp bit for bit).
struct ScoreReq { const int32_t* lengths; int64_t ignore_id; float* token_lp; int ld_lp; float* row_sum; int32_t* row_cnt; int64_t* top1_ids; float* top1_lp; TopkAttach topk{}; };
inline hipError_t launch_score(const HeadWeight& hw, const bf16_t* xb, const int64_t* ids, int ld_ids, int rows, int T, float* amax_val,
                               int* amax_idx, float* amax_sum, float* scratch, const ScoreReq& q, hipStream_t s) {
    SkinnyArgs ha;
    vocab_head_args(ha, hw, xb, rows, T, true, nullptr, amax_val, amax_idx, amax_sum);
    const HeadTargets tg{ids, T, ld_ids, 1, scratch};
    hipError_t e = launch_skinny(ha, SK_BIAS_F32, s, &tg);
    if (e != hipSuccess) return e;
    const ScoreOut o{q.token_lp ? q.token_lp : scratch + (size_t)rows * T, q.token_lp ? q.ld_lp : T - 1, q.row_sum, q.row_cnt, q.top1_ids, q.top1_lp};
    e = launch_score_final(amax_val, amax_idx, amax_sum, (hw.V + 15) / 16, scratch, ids, ld_ids, rows, T, q.lengths, q.ignore_id, hw.V, o, s);
    if (e != hipSuccess || !q.topk.k) return e;
    HeadTopkArgs ta{};
    ta.X = xb; ta.ldx = hw.D; ta.hw = hw; ta.val = amax_val; ta.idx = amax_idx; ta.sum = amax_sum;
    ta.rows = rows; ta.T = T - 1; ta.row_stride = T; ta.row_off = 0;
    ta.k = q.topk.k; ta.top_ids = q.topk.ids; ta.top_lp = q.topk.lp; ta.ld = q.topk.ld;
    return launch_head_topk(ta, s);
}
// One pass of a handle's decoder stack over text rows, and what its vocabulary head produces (host only; the request of both
// handles' text_forward, gitcap.hip and student.hip -- the teacher's TextReq adds what only its stack takes).
struct RowsReq {
    // which rows and positions: ids [rows][ld_ids], query positions t0 .. t0 + T - 1 (K/V of earlier positions come from the cache)
    const int64_t* ids = nullptr; int ld_ids = 0, rows = 0, t0 = 0, T = 0;
    // what the head produces; none of logits_out / argmax_out / score: the stack's rows only, no head
    float* logits_out = nullptr;                    // nullable: fp32 logits
    int64_t* argmax_out = nullptr; int ld_argmax = 0;   // nullable: the last position's arg-max of every row (launch_argmax_final's out)
    int32_t* sep_cnt = nullptr; int step = 0;       // launch_argmax_final's
    float* lp_out = nullptr; int ld_lp = 0;         // nullable, needs argmax_out: the token's log-probability
    const ScoreReq* score = nullptr;                // nullable: all positions through launch_score instead
    // k != 0, needs argmax_out: the k best columns of the row the arg-max reads (launch_head_topk behind the arg-max launch; the head
    // runs its LSE form); ids / lp point at this position's entries of row 0, ld = the row pitch in positions
    TopkAttach topk{};
    // nullable, needs argmax_out (a prompted greedy loop): the arg-max launch's prompt; it writes position t0 + T
    const PromptArgs* prompt = nullptr;
};

// ---- candidate generation and the beam state of the search loops (search.hip) ------------------------------------------------------
// The candidates of one search step, what launch_beam_topk (the K best) and launch_sample_rows (draws) have in common: B * beams rows
// of logits [.][ld] (V columns) ranked under log_softmax + beam_scores; candidate slots out_scores / out_idx [B][K] (K = beams * pn
// for draws).
struct CandArgs {
    const float* logits; int ld;
    const float* beam_scores;
    // rp != 1.0f: the same ranking under a repetition penalty (model.py:522-531): every logit whose column occurs in the row's prefix
    // prefix_ids[row * ld_ids + 0 .. cur_len - 1] (int64; ids outside [0, V) are ignored) becomes x < 0 ? x * rp : x / rp, once however
    // often the token occurs, and the log-softmax is that of the penalised row.  rp == 1.0f: the prefix is neither checked nor read.
    const int64_t* prefix_ids; int ld_ids, cur_len; float rp;
    int B, beams, V;
    float* out_scores; int* out_idx;
    // bn (nullable): row b * beams + j of the mask bans columns of that beam row before the penalty, the chunk statistics and the
    // chunk's top K (the BAN forms of the chunk kernel, combinable with the penalty): the log-softmax is that of the banned row;
    // draws: banned columns are -inf before the penalty, the temperature and the filter -- the BAN form of the kernel.
    const HeadBan* bn;
};
// top-K over (beam, vocab) of log_softmax(logits) + beam_scores per batch element: sorted descending, ties by smaller flat index
// j*V + v.  Logits of -inf are no candidates; where a clip has fewer than K candidates the remaining slots hold the sentinel
// (score -inf, index 0x7fffffff) -- launch_beam_step divides the index by V and must never be handed one.
size_t beam_topk_scratch_bytes(int B, int beams, int V, int K);   // device scratch launch_beam_topk needs (V <= 131072)
hipError_t launch_beam_topk(const CandArgs& c, int K, void* scratch, hipStream_t s);
// the sampling branch of the search (model.py:532-554) for B * beams rows: penalty, temperature, top-k / top-p filter
// (min_tokens_to_keep = 2), pn draws without replacement per row from a counter-based Philox stream (seed, row, cur_len, column);
// candidate p = j * pn + d of clip b = draw d of row b * beams + j, flat index (p % beams) * V + word, unsorted (search.hip).
// opt = the call's SampleOpt (host_logic.h; `on` is not read).
// kept_out (int [B*beams]) / logz_out (fp32 [B*beams]): columns the filter kept / log-sum-exp of the filtered row; nullable.
struct SampleStats { int* kept_out; float* logz_out; };
hipError_t launch_sample_rows(const CandArgs& c, int pn, const SampleOpt& opt, const SampleStats& st, hipStream_t s);
// One workgroup per row builds the row's ban mask from scratch (every word of the row is written: the buffer is reused every
// step): the union of
//   n-gram (n >= 1; HF NoRepeatNGramLogitsProcessor): prefix[i + n - 1] for every i in 0 .. cur_len - n whose n - 1 tokens
//           prefix[i .. i + n - 2] equal the last n - 1 tokens of the prefix (n = 1: every token of the prefix);
//   length: sep_id while cur_len < min_length (HF MinLengthLogitsProcessor);
//   suppress: the n_suppress ids of the device list (int32, duplicates allowed).
// prefix = ids[row * ld_ids + 0 .. cur_len - 1], compared as values; an id outside [0, V) bans nothing.  Bits of the last word
// beyond V and the words behind ceil(V / 16) are 0.  V <= 131072 (the row's bitmap is built in LDS), n_suppress <= 256.
hipError_t launch_ban_mask(const int64_t* ids, int ld_ids, int rows, int cur_len, int n, int min_length, int sep_id,
                           const int32_t* suppress, int n_suppress, int V, uint16_t* mask, int ld_mask, hipStream_t s);
// The same kernel body with the rules read on the device when the kernel runs, from rec int32 [BAN_REC_WORDS]: rec[0] = n, rec[1] =
// min_length, rec[2] = n_suppress (clamped on the device to 0 .. BAN_REC_MAX_SUPPRESS: no value reads past the record), rec[3] = 0,
// rec[4 ..] = the ids.  Nothing of the rules is a kernel argument, so a captured launch follows the record written last (the
// student's token loops, student.hip); cur_len, sep_id, V and the id rows stay arguments.  The mask is launch_ban_mask's, bit for bit.
constexpr int BAN_REC_HEADER = 4, BAN_REC_MAX_SUPPRESS = 256, BAN_REC_WORDS = BAN_REC_HEADER + BAN_REC_MAX_SUPPRESS;
hipError_t launch_ban_mask_rec(const int64_t* ids, int ld_ids, int rows, int cur_len, int sep_id, const int32_t* rec, int V, uint16_t* mask,
                               int ld_mask, hipStream_t s);
// device-resident beam search state + one bookkeeping step per decoder step
struct BeamBuffers {
    int64_t *ids0, *ids1, *words, *hyp_ids;
    float *beam_scores, *hyp_score;
    int32_t *src_rows, *done, *hyp_len;
};
// n finished hypotheses per clip (1 <= n <= 16): hyp_ids [B][n][max_len], hyp_score / hyp_len [B][n], stored in storage order in
// slots 0 .. cnt - 1, hyp_len 0 behind them (launch_beam_init zeroes all B * n).  step: n = 1 runs beam_step_kernel, n > 1 the n-slot kernel.
// finish: decoded [B][n][max_len] / logprobs [B][n] by descending score; first_*: rank 0 again as [B][max_len] / [B]; all nullable.
hipError_t launch_beam_init(const BeamBuffers& bb, int B, int beams, int n, int max_len, int cls, hipStream_t s);
struct BeamStepArgs {
    int n;                                      // hypothesis slots per clip
    const float* cand_scores; const int* cand_idx;   // [B][K]: launch_beam_topk's or launch_sample_rows'
    int B, beams, K, V;
    int cur_len, max_len, eos; float length_penalty;
    int cur;                                    // which of ids0 / ids1 holds the current prefixes
    // sampled: the candidates are draws (launch_sample_rows), in no order: is_done takes the maximum of the K scores, the candidates
    // are walked as given, and a clip left with 0 < kept < beams live beams pads only the missing ones with (0, eos, row 0); any n >= 1.
    bool sampled;
    // prompt (nullable; rows = clips): a clip with cur_len < lengths[b] is forced -- every beam keeps its prefix and appends
    // ids[b][cur_len], src_rows is the identity, beam_scores / done / the hypothesis slots are untouched, the candidates are not
    // read; with cur_len >= max_len (the prompt's) the launch is the one without a prompt.
    const PromptArgs* prompt;
};
hipError_t launch_beam_step(const BeamBuffers& bb, const BeamStepArgs& a, hipStream_t s);
struct BeamFinishOut { int64_t* decoded; float* logprobs; int64_t* first_decoded; float* first_logprobs; };
hipError_t launch_beam_finish(const BeamBuffers& bb, int n, int B, int max_len, int eos, const BeamFinishOut& o, hipStream_t s);

// ---- attention (attention.hip) ------------------------------------------------------------
// Full (unmasked) self-attention over groups of S rows: qkv [G*S][3*W] bf16 (q | k | v, head h
// at columns h*64), ctx [G*S][W] bf16.  Used for the ViT frames (S = N) and for the image
// prefix of the decoder (S = F*N).
hipError_t launch_attn_full(const bf16_t* qkv, bf16_t* ctx, int G, int S, int H, hipStream_t s);
// Variable-length form (a ragged batch's decoder image prefix): group g = rows off[g] .. off[g] + len[g] - 1 of the packed
// qkv / ctx (device int32 [G], 1 <= len[g] <= S_max; S_max sizes the grid).  Each group's ctx rows are bit for bit those of
// launch_attn_full(G = 1, S = len[g]) on the group alone; no row outside the groups is written.
hipError_t launch_attn_full_varlen(const bf16_t* qkv, bf16_t* ctx, int G, const int32_t* off, const int32_t* len, int S_max, int H, hipStream_t s);

// Attention sub-layer for text rows (txtblock.hip): query (r, t0+j) attends the image keys of clip r/beams and the text
// keys 0..t0+j of row r -> this head's share of the output dense -> the last head of a row to arrive adds bias +
// residual and applies LayerNorm.  One workgroup per (text row, head).
struct TxtBlockArgs {
    const bf16_t* kv_img;                       // [B*S_img][3D] this layer
    const bf16_t* kv_txt;                       // [R][Tmax][3D] this layer (q | k | v of the text rows)
    int rows, beams, t0, T, Tmax, S_img, H, D;
    const void* aow;                            // output dense [D][D]: bf16, or e4m3 bytes when aoscale != nullptr
    const void* aowpk;                          // nullable (bf16 only): its fragment-major copy (launch_pack_frags)
    const float* aoscale;                       // nullable: [D] per-row power-of-two scale of e4m3 weights
    const float *aob, *g1, *b1;                 // its bias; LayerNorm of the sub-layer
    const float* xin;                           // [M][D] the sub-layer's input (residual)
    float eps;
    float* part;                                // [M][H][D] fp32 per-head partials of the output dense
    unsigned* cnt;                              // [M] arrival tickets (zero between launches)
    float* xs; bf16_t* xsb;                     // out: x1 [M][D] fp32 and bf16 (xs may alias xin)
    // opt-in kv_cache = v_e4m3: V of the image keys as e4m3 codes [H][v8_pitch][64] + one power-of-two scale per (key, head)
    // [H][v8_pitch], head-major (launch_kv_quant_v); K and the text rows' own K/V stay bf16.  nullptr: bf16 V from kv_img.
    const unsigned char* v8_img; const float* vs_img; int64_t v8_pitch;
    int Mh;                                     // set by the launcher
    int nt_kv;                                  // 1: the K/V rows are streamed with non-temporal loads (they do not fit the caches anyway)
    // variable-length form (both or neither; device int32 [clips]): clip c's image keys are the rows off[c] .. off[c] + len[c] - 1
    // of the packed kv_img / v8_img / vs_img, S_img is not read.  nullptr: every clip has S_img rows at c * S_img.
    const int32_t *off, *len;
};
bool txt_block_ok(int D);
extern std::atomic<bool> g_txt8;                                          // txtblock.hip: 8-wave workgroups where units > CUs (speed switch 9)
hipError_t launch_txt_block(const TxtBlockArgs& a, hipStream_t s);

// Per-token attention maps from the cached q | k of a text pass (attnmap.hip): two launches on `s`.  kv_txt [L][.][Tmax][3D] and
// kv_img [L][.][3D] with their layer strides in elements; rows text rows of T filled positions (from position 0), rows_per_clip rows
// per clip; N image tokens per frame; dense: clip c's S_img (== Smax) image rows at c * S_img; off / len (both or neither, device
// int32 [clips]): rows off[c] .. off[c] + len[c] - 1, len[c] a multiple of N and <= Smax.  layer: -1 the mean over all L, or one.
// lengths (nullable, device int32 [rows]): positions >= lengths[r] are written as zeros.  stats: attn_map_scratch_floats() floats.
// Out: frame_mass [rows][T][ld_f] (columns 0 .. Smax / N - 1), text_mass [rows][T], patch_map (nullable) [rows][T][ld_s] (columns
// 0 .. Smax - 1); columns beyond the widths are not written.
struct AttnMapArgs {
    const bf16_t* kv_img; size_t img_layer_stride;
    const bf16_t* kv_txt; size_t txt_layer_stride;
    int L, H, D, rows, rows_per_clip, T, Tmax, N, S_img, Smax;
    const int32_t *off, *len;
    int layer;
    const int32_t* lengths;
    float* stats;
    float* frame_mass; int ld_f;
    float* text_mass;
    float* patch_map; int ld_s;
};
size_t attn_map_scratch_floats(int L, int H, int rows, int T, int layer);
hipError_t launch_attn_map(const AttnMapArgs& a, hipStream_t s);

// Small attention of the student decoder (student.hip): one wave per (query row, head), at most 64 keys,
// any head_dim that is a multiple of 8 (<= 128).  Query m = (r, j), r = m / T: q at
// q + (r*q_row_stride + q_row_off + j)*ldq + h*hd; key/value i of row r at k|v + (r*keys_stride + i)*ldkv + h*hd.
// nkeys > 0: every query sees keys 0..nkeys-1 (cross-attention); nkeys == 0: causal, keys 0..t0+j.
// ids != nullptr: key i of row r is masked when ids[r*ld_ids + i] == pad_id (all keys masked -> NaN, as torch).
struct SmallAttnArgs {
    const bf16_t* q; int ldq, T, q_row_stride, q_row_off;
    const bf16_t* k; const bf16_t* v; int ldkv, keys_stride, nkeys, t0;
    const int64_t* ids; int ld_ids, pad_id;
    bf16_t* ctx; int ldc;
    int M, H, hd;
};
hipError_t launch_attn_small(const SmallAttnArgs& a, hipStream_t s);
// The probabilities of attn_small's cross-attention form (student.hip: cross_probs_kernel), the per-frame attribution of the student
// (one memory token per frame): one wave per (query m, head), q row m of q (ldq), keys 0 .. F - 1 of row r = m / T at
// k + (r * keys_stride + i) * ldkv, head h at columns h * hd: probs [M][H][F] fp32 = softmax(q . k / sqrt(hd)), attn_small's own
// arithmetic.  F <= 64, hd % 8 == 0, hd <= 128.
struct CrossProbsArgs {
    const bf16_t* q; int ldq, T;
    const bf16_t* k; int ldkv, keys_stride, F;
    float* probs;
    int M, H, hd;
};
hipError_t launch_cross_probs(const CrossProbsArgs& a, hipStream_t s);
// The variable-length forms of the two (clips of different length, gitcap_student_attach_frame_counts): the keys of decoder row r
// are rows key_off[r] .. key_off[r] + key_len[r] - 1 (1 <= key_len <= 64) of the PACKED k | v -- device int32 tables of M / T
// entries, read at run time -- in place of r * keys_stride .. + nkeys - 1; a.keys_stride, a.nkeys and a.t0 are not read, a.ids must
// be null.  A row with key_len = n has the bits of the plain launch at nkeys = n.  cross_probs: probs stays [M][H][a.F], the
// columns from key_len[r] on hold 0.
hipError_t launch_attn_small_varlen(const SmallAttnArgs& a, const int32_t* key_off, const int32_t* key_len, hipStream_t s);
hipError_t launch_cross_probs_varlen(const CrossProbsArgs& a, const int32_t* key_off, const int32_t* key_len, hipStream_t s);
// frame_mass [rows][T][ld_f] (columns 0 .. F - 1) = the mean of probs [L][rows * T][H][F] over the heads and the selected layers
// (layer = -1: all, ascending; heads ascending: a fixed order); zeros at positions j >= lengths[r] (nullable, device int32 [rows])
hipError_t launch_cross_mean(const float* probs, int L, int rows, int T, int H, int F, int layer, const int32_t* lengths,
                             float* frame_mass, int ld_f, hipStream_t s);
// x[m] = (embed[ids[r*ld_ids + t0 + j]] + pe[t0 + j]) / sqrt(D), m = r*T + j  -> xf (fp32) and xb (bf16)
hipError_t launch_student_embed(const int64_t* ids, int ld_ids, int rows, int T, int t0, const float* embed,
                                const float* pe, int D, int vocab, float* xf, bf16_t* xb, hipStream_t s);
// The start of a prompted student loop (gitcap_student_attach_prompt; student.hip: student_prompt_stage_kernel): ids [rows][ld] row r =
// CLS, tokens 1 .. len - 1 of prm_ids [rows / k][ld_prm] row r / k, CLS behind them; len = prm_len[r / k] clamped to [1, max_len]
// (max_len <= ld_prm and <= ld: no read leaves a table row, every column of a row is written).  lp (nullable, [rows][ld_lp]):
// columns 0 .. pmin - 2 = 0.0f (1 <= pmin <= ld_lp + 1).  k = 1: the greedy loop's rows; k beams of a clip share its prompt.
struct StudentPromptStageArgs {
    const int64_t* prm_ids; int ld_prm; const int32_t* prm_len;
    int rows, k, max_len; int64_t cls;
    int64_t* ids; int ld;
    float* lp; int ld_lp, pmin;
};
hipError_t launch_student_prompt_stage(const StudentPromptStageArgs& a, hipStream_t s);
// The bookkeeping step of the student's beam search (student.hip: student_beam_step_kernel): the candidates [B][k] (flat index =
// beam * V + token, best first) of the step that decoded position t become rows b * k + j of ids_next (prefix 0 .. t of the source row
// of ids_cur, the token at t + 1; ld >= t + 2), scores and src_rows.  prompt (nullable; rows = clips): a clip with t + 1 < lengths[b]
// keeps every row's own prefix, appends ids[b][t + 1], src_rows the identity, scores untouched, candidates unread; with
// t + 1 >= max_len (the prompt's) the launch is the one without a prompt.
struct StudentBeamStepArgs {
    const float* cand_scores; const int* cand_idx;
    const int64_t* ids_cur; int64_t* ids_next;
    float* scores; int32_t* src_rows;
    int B, k, V, t, ld;
    const PromptArgs* prompt;
};
hipError_t launch_student_beam_step(const StudentBeamStepArgs& a, hipStream_t s);

// ---- row ops (rowops.hip) -----------------------------------------------------------------------------
struct LnArgs {
    const float* x; int ldx;      // [rows][ldx]
    const float* gamma; const float* beta; float eps;
    int rows, D;
    float* out_f32; int ld_f32;   // nullable
    bf16_t* out_bf16; int ld_bf16;// nullable
    const float* add_vec;         // nullable: out += add_vec[((row / add_div) % add_mod) * D + c]
    int add_div, add_mod;
    // optional SECOND LayerNorm of the first one's fp32 output (canonical widths only): out_f32 = LN(x), out_bf16 =
    // LN2(LN(x)) -- ln_pre and the first block's LN1 of the ViT in one pass over the rows.  Same bits as two launches.
    const float* gamma2; const float* beta2; float eps2;
    // optional: rows with row % cls_period == 0 are not read from x but are cls[c] + cls_pos[c] (the CLS token + its position
    // embedding of the ViT front end: x[frame * N] of model.py:378's encoder input) -- the row a cls_rows launch would write
    const float* cls; const float* cls_pos; int cls_period;
};
hipError_t launch_layernorm(const LnArgs& a, hipStream_t s);

// frames [nf][3][H][W] f32 -> patches bf16 [nf*G*G][Kp] (k = c*p*p + py*p + px, zero padded)
hipError_t launch_im2col(const float* frames, bf16_t* patches, int nf, int img, int p, int Kp, hipStream_t s);
// out[b][e][s][:] = s < S_img ? img[e][b*S_img + s][:] : txt[e][b*T + s - S_img][:]   (e < n_entries; fp32 rows of D)
hipError_t launch_gather_hidden(const float* img, const float* txt, float* out, int n_entries, int B, int S_img, int T, int D,
                                size_t img_entry_stride, size_t txt_entry_stride, hipStream_t s);
// V slice of kv [rows][3D] (bf16) -> e4m3 codes v8 [H][pitch][64] + power-of-two scales vs [H][pitch] per (row, head), head-major
hipError_t launch_kv_quant_v(const bf16_t* kv, unsigned char* v8, float* vs, int rows, int D, int H, int64_t pitch, hipStream_t s);
// frame window (gitcap_window_*): ring = fp32 ln_post rows of the last F frames of B clips, [B][F][rows_per_frame][D] (no temporal
// embedding).  scatter: src [B][n][rows_per_frame][D] (contiguous) -> ring slot (head + j) % F of clip b, frame j of the push.
hipError_t launch_window_scatter(const float* src, float* ring, int B, int n, int F, int head, int rows_per_frame, int D, hipStream_t s);
// assemble: window position f of clip b = ring slot (head + f) % F (head = the oldest frame) + temporal[f] (nullable) -> out bf16
// [B*F*N][D] (the decoder input) and vis fp32 (nullable); the same bits as the ln_post epilogue that adds the embedding itself
hipError_t launch_window_assemble(const float* ring, const float* temporal, bf16_t* out, float* vis, int B, int F, int head, int N, int D,
                                  hipStream_t s);
// Ragged batches (gitcap_attach_frame_counts): clips of 1..255 frames each, packed clip-major.  RaggedCounts (host_logic.h) travels
// by value (a stream-ordered launch captures it), launch_ragged_tables writes off[b] = N * sum_{i<b} n[i], len[b] = N * n[b]
// (int32 [B]) and pos[frame] = the frame's index inside its clip (int32 [sum n]).
hipError_t launch_ragged_tables(const RaggedCounts& rc, int N, int32_t* off, int32_t* len, int32_t* pos, hipStream_t s);
// row r (frame r / N) of the decoder input = bf16(ln[r] + temporal[pos[r / N]]), optionally also the fp32 sum (visual features):
// window_assemble's add and rounding, i.e. the fused ln_post epilogue's, with the frame's position read from a table
hipError_t launch_ragged_temporal(const float* ln, const float* temporal, const int32_t* pos, bf16_t* out, float* vis, int frames, int N,
                                  int D, hipStream_t s);
// Stream pool (gitcap_pool_*): ring = fp32 ln_post rows of n_streams independent windows, [ring_frames][N][D] (no temporal
// embedding), ring frame = stream * F + slot.  The tables are device int32 the host planned (host_logic.h: pool_plan): every entry
// in range, no destination twice.
// scatter: packed frame i of stage [frames][N][D] -> ring frame dst[i]
struct PoolScatterArgs { const float* stage; float* ring; const int32_t* dst; int frames, N, D; };
hipError_t launch_pool_scatter(const PoolScatterArgs& a, hipStream_t s);
// assemble: row (g, tok) of out bf16 [frames * N][D] = ring[src[g]][tok] + temporal[pos[g]] (temporal nullable: no add);
// window_assemble's / ragged_temporal's add and rounding
struct PoolAssembleArgs { const float* ring; const float* temporal; const int32_t *src, *pos; bf16_t* out; int frames, N, D; };
hipError_t launch_pool_assemble(const PoolAssembleArgs& a, hipStream_t s);
// f32 -> bf16 copy
hipError_t launch_cast_bf16(const float* in, bf16_t* out, int64_t n, hipStream_t s);
// e4m3 weight rows [rows][K] (+ per-row power-of-two scale) -> bf16 [rows][K] (exact); K % 16 == 0
hipError_t launch_dequant_fp8(const unsigned char* w8, const float* scale, bf16_t* out, int rows, int K, hipStream_t s);
// up to four such matrices in ONE launch (the weights of a transformer layer); n16[i] = rows_i * K_i / 16
struct DequantBatch { const unsigned char* w8[4]; const float* scale[4]; bf16_t* out[4]; int K[4]; int64_t n16[4]; int n; };
hipError_t launch_dequant_fp8_batch(const DequantBatch& b, hipStream_t s);
// fragment-major copy of a GEMM weight [rows16][K] (bf16: elem_bytes 2, e4m3 codes: 1) for the weight-streaming text kernels
hipError_t launch_pack_frags(const void* src, void* dst, int rows16, int K, int elem_bytes, hipStream_t s);
hipError_t launch_gather_txt_rows(const bf16_t* src, bf16_t* dst, const int32_t* src_rows, int rows,
                                  int t_len, int Tmax, int width, int layers, size_t layer_stride, hipStream_t s);

// ---- preprocessing (preproc.hip) -----------------------------------------------------------------------------------------------
// uint8 HWC BGR frames [nf][H][W][3] -> CLIP-normalised fp32 NCHW [nf][3][crop][crop] (bicubic resize + centre crop)
hipError_t launch_preprocess(const unsigned char* in, float* out, int nf, int H, int W, int crop, hipStream_t s);
// the same transform fused with the patch gather: -> bf16 patch rows [nf*G*G][Kp] (layout of launch_im2col)
hipError_t launch_preprocess_patches(const unsigned char* in, bf16_t* patches, int nf, int H, int W, int crop, int p, int Kp, hipStream_t s);
// the same transform fused with the gather of a 3x3 stride-2 pad-1 convolution over the cropped frame (TinyViT's first stem conv):
// -> bf16 im2col rows [nf*(crop/2)^2][32], k = ci*9 + ky*3 + kx, every column written (zero at outside taps and k >= 27); crop even
hipError_t launch_preprocess_stem(const unsigned char* in, bf16_t* col, int nf, int H, int W, int crop, hipStream_t s);
