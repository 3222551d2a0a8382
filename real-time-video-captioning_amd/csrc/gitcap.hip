// libgitcap C ABI: handle, weights, workspace and the launch sequences of the GIT caption path.
// Declarations and the reference call each entry point replaces: include/gitcap.h.
#include "../../include/gitcap.h"
#include "kernels.h"
#include "host_util.h"
#include "student_internal.h"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include <sched.h>

#define GITCAP_ABI_VERSION 1

// Speed-only switches (results do not depend on them: tests/test_parity_gpu.py).  Process-wide, set once from the
// environment; gitcap_dbg_config (a test hook) may flip them at run time, so they are atomics: an entry point running on
// another thread reads a consistent value at each use and either value gives the same bits.
// g_row_prologue is shared with student.hip.
std::atomic<bool> g_row_prologue{!env_flag("GITCAP_NO_ROW_PROLOGUE")};
std::atomic<bool> g_head_share{!env_flag("GITCAP_NO_HEAD_SHARE")};        // kernels.h; gitcap_dbg_config(10, .)
// a prompted greedy loop runs the positions every row's prompt covers as ONE multi-position pass (gitcap_dbg_config(20, 0): as
// forced token steps, the plan of a ragged batch whose shortest prompt is the lone CLS; same ids either way)
std::atomic<bool> g_prompt_prefill{true};         // kernels.h: shared with student.hip, as g_row_prologue is
std::atomic<bool> g_rows3{!env_flag("GITCAP_NO_ROWS3")};                  // kernels.h; gitcap_dbg_config(11, .)

// compute units of the current device, cached per device (the workgroup -> tile maps and the tile-height choice depend on it)
int device_cus() {
    static std::atomic<int> cache[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 256;
    std::atomic<int>& c = cache[dev & 63];
    int v = c.load(std::memory_order_relaxed);
    if (v <= 0) {
        int n = 0;
        v = (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0) ? n : 256;
        c.store(v, std::memory_order_relaxed);
    }
    return v;
}

namespace {

// a GEMM weight [Npad16][K]: bf16, or OCP e4m3 bytes + one power-of-two scale per row (scale != nullptr)
struct WRef {
    const void* p = nullptr; const float* scale = nullptr;
    const void* pk = nullptr;          // fragment-major copy for the weight-streaming text kernels (launch_pack_frags), or null
    // rows n0.. of the matrix (K columns); n0 a multiple of 16
    WRef rows_from(size_t n0, size_t K) const {
        WRef r; r.p = (const char*)p + n0 * K * (scale ? 1 : 2); r.scale = scale ? scale + n0 : nullptr;
        r.pk = pk ? (const char*)pk + n0 * K * (scale ? 1 : 2) : nullptr;      // whole 16-row tiles: the same byte offset
        return r;
    }
};
struct EncLayer {
    const float *ln1w, *ln1b, *ln2w, *ln2b, *qkvb, *projb, *fc1b, *fc2b;
    WRef qkvw, projw, fc1w, fc2w;
};
struct DecLayer {
    const float *qkvb, *aob, *ln1w, *ln1b, *fc1b, *fc2b, *ln2w, *ln2b;
    WRef qkvw, aow, fc1w, fc2w;
};

}  // namespace

struct gitcap : HandleCore {
    gitcap_config c;
    std::map<std::string, DevTensor> w;
    std::map<std::string, float*> wscale;          // e4m3 storage: per-row scales of the GEMM weights
    std::map<std::string, std::pair<void*, size_t>> wpack;   // fragment-major copies of the text-path weights (name -> buffer, bytes)
    bool finalized = false, fp8 = false;
    bf16_t* wstage = nullptr;                       // e4m3 storage: bf16 staging panel of a single GEMM
    bf16_t* lstage = nullptr;                       // e4m3 storage: bf16 staging of the (up to 4) matrices of one layer
    size_t lstage_elems = 0;
    const void* staged_src[4] = {nullptr, nullptr, nullptr, nullptr};   // which e4m3 matrices lstage currently holds, and where
    const bf16_t* staged_dst[4] = {nullptr, nullptr, nullptr, nullptr};
    int n_staged = 0;
    // opt-in export of the decoder's per-layer hidden states (gitcap_hidden_states_enable): [L+1][rows][D] fp32
    bool want_hidden = false;
    float *hid_img = nullptr, *hid_txt = nullptr;
    int hid_T = 0;
    float* enc_tap = nullptr;                       // gitcap_dbg_enc_tap: caller's buffer for the ViT's residual stream per block
    int64_t weight_bytes = 0;

    // derived sizes
    int N = 0, G = 0, Kp = 0, Dv = 0, D = 0, V = 0, Vp = 0;
    int Smax = 0, Mi = 0, Pp = 0, R = 0, Tmax = 0, Mt = 0;

    // workspace (image rows)
    float *x = nullptr, *tmp = nullptr;
    float2* ln_stats = nullptr;         // [Mi][16] LayerNorm segment statistics exchanged inside the fused GEMMs
    unsigned* ln_cnt = nullptr;         // [Mi / 256][2] {arrivals, generation} per 256-row block (self-resetting barrier)
    size_t ln_cnt_words = 0;
    unsigned* ln_fail = nullptr;        // host-pinned word a fused launch raises when a tile gave up waiting (gemm_epilogue.h)
    ExchangeHealth xh;                  // host_logic.h: once raised, the handle runs GEMM + row kernel for good
    int cus = 256;                      // compute units of the handle's device
    int nslab_max = 16;                 // fp32 split-K slabs per text row the workspace holds
    // opt-in fp8 MFMA compute of the image rows' FFN GEMMs (gitcap_set_compute; gemm256.hip): e4m3 activation operands
    bool f8ffn = false;
    float f8_scale = 1.0f / 16.0f;                   // static power-of-two scale of the e4m3 activation codes (gitcap_set_fp8_scale)
    unsigned long long* f8_sat = nullptr;            // device counter: codes of valid rows the producing epilogues clamped at +-448
    unsigned char *hb8 = nullptr, *ffn8 = nullptr;   // [Mi][Dm] LayerNorm output / [Mi][Fm] GELU output as e4m3 codes of value * 16
    bf16_t *hb = nullptr, *qkv = nullptr, *ctx = nullptr, *ffn = nullptr, *patches = nullptr;
    // opt-in kv_cache = v_e4m3 (gitcap_set_kv_cache): V of the image prefix as e4m3 codes [layer][Mi][D] + power-of-two scales
    // [layer][Mi][H] per (token, head), written behind every decoder layer's q|k|v GEMM of the image rows, read by txt_block
    bool kv_v8 = false;             // (the codes and scales are the slots' v8_img / vs_img)

    // resolved weights
    WRef patch_w, vproj_w, head_w;
    const float *cls = nullptr, *pos = nullptr, *ln_pre_w = nullptr, *ln_pre_b = nullptr, *ln_post_w = nullptr,
                *ln_post_b = nullptr, *temporal = nullptr, *vproj_b = nullptr, *vproj_lnw = nullptr,
                *vproj_lnb = nullptr, *word = nullptr, *tpos = nullptr, *txt_lnw = nullptr, *txt_lnb = nullptr,
                *head_b = nullptr;
    std::vector<EncLayer> enc;
    std::vector<DecLayer> dec;

    // Four slots (image-prefix K/V, text-row workspace, stop counters; two decode streams shared by the slots).  While one
    // batch's image pass (MFMA bound) runs on `s_enc`, the token loops of the batches submitted before
    // it (chains of tiny latency-bound kernels) interleave on the decode streams (slot i on stream i % n_txt)
    // (gitcap_greedy_submit / _wait).  The synchronous entry points always use slot 0 on the caller's
    // stream; they first make that stream wait for every submission still in flight (join_async).
    struct Slot {
        bf16_t* kv_img = nullptr; int32_t* sep_cnt = nullptr;
        unsigned char* v8_img = nullptr; float* vs_img = nullptr;   // kv_cache = v_e4m3
        // text-row workspace of the slot (token loops of different slots may run concurrently)
        float *xs = nullptr, *xs2 = nullptr, *slabs = nullptr, *part = nullptr, *amax_val = nullptr; int* amax_idx = nullptr;
        float* amax_sum = nullptr;          // third head partial, [Mt][ntiles] like amax_val: allocated by the first gitcap_attach_token_logprobs
        float* score_buf = nullptr;         // gitcap_score (slot 0 only, first use): [2][Mt] target logits, lp rows the caller did not ask for
        unsigned* row_cnt = nullptr;
        bf16_t *xsb = nullptr, *fs = nullptr, *kv_txt = nullptr, *kv_txt2 = nullptr;
        // device-resident beam-search state of the slot (gitcap_beam_search / _submit)
        BeamBuffers beam{};
        float* beam_logits = nullptr;       // [R][V]
        float* cand_scores = nullptr;       // [B][16]
        int* cand_idx = nullptr;
        uint16_t* ban_mask = nullptr;       // constrained decoding: [R][ban_ld] ban mask of the step's rows; allocated by the first gitcap_attach_constraints
        char* topk_scratch = nullptr;       // beam_topk chunk statistics + per-chunk candidates (sized for max_batch x max_beams rows)
        // n-best hypotheses of the search (num_keep_best > 1): [max_batch][16][Tmax + 1] ids, [max_batch][16] scores and lengths;
        // allocated by the first gitcap_attach_search_options that asks for more than one
        int64_t* nb_ids = nullptr; float* nb_score = nullptr; int32_t* nb_len = nullptr;
        int B = 0, S = 0;                   // clips and image rows per clip of the image prefix the slot holds (have: it holds one)
        // ragged (gitcap_attach_frame_counts): clip b's image rows are off[b] .. off[b] + len[b] - 1 of the packed rows (device
        // int32 [max_batch]), S is the largest len[b]; fpos [max_batch * max_frames] = each packed frame's index inside its clip.
        // S_tot = the image rows the slot holds, B * S of a dense prefix.
        int32_t *off = nullptr, *len = nullptr, *fpos = nullptr;
        int S_tot = 0;
        bool ragged = false;
        bool have = false, used = false;
        int Mt = 0;             // text rows (rows x positions) the slot's row workspace holds
        // draft verification (gitcap_greedy_draft; slot 0 only, first use): launch_draft_accept_rows' scratch -- tok / lp_tok int[Mt],
        // row_res int[2 * max_batch], ticket [1 + max_batch] (zero between launches) -- and keep_len int32[max_batch], the rows'
        // verified lengths the KEEP arg-max of the tail reads
        int *acc_tok = nullptr, *acc_lp = nullptr, *acc_row = nullptr;
        unsigned* acc_ticket = nullptr;
        int32_t* keep_len = nullptr;
        hipEvent_t ev_in = nullptr, ev_enc = nullptr, ev_dec = nullptr;
        hipStream_t s_txt = nullptr;
    };
    static constexpr int NSLOT = 4;
    Slot slots[NSLOT];
    int cur_slot = 0, next_ticket = 0;      // cur_slot: the slot the launches being issued work on (select_slot)
    int poison_upto = 0;    // tickets below this were in flight when the statistics exchange failed: their results are undefined
    hipStream_t s_enc = nullptr;
    hipStream_t txt_streams[NSLOT] = {nullptr, nullptr, nullptr, nullptr};   // owned; slot i decodes on txt_streams[i % n_txt]
    int n_txt = NSLOT;
    bool pipelined = false; // the launches being issued belong to a gitcap_greedy_submit (other batches share the chip)
    // The one-shot attachments (CallOpts, host_logic.h).  pending: what the gitcap_attach_* setters wrote and no call has taken yet:
    // log-probabilities go to the next greedy-family call, search options + sampling to the next beam-family call, prompt and
    // constraints to the next call of either family, frame counts to the next call that runs an image pass (calls that cannot
    // take them refuse).  call: the options of the call whose launches are being issued (as cur_slot / pipelined), installed by
    // the entry point's CallScope and empty outside it.  ban_ld: words per row of the constraints' ban mask
    CallOpts pending{}, call{};
    int ban_ld = 0;
    // gitcap_greedy_draft: acc_host = the accept launch's page-locked words (int32 [4 + max_batch]: min covered, max covered,
    // accepted summed, fired, then accepted per row), acc_ev = the event the call waits for behind it; gitcap_draft_stats' counters
    int32_t* acc_host = nullptr;
    hipEvent_t acc_ev = nullptr;
    int64_t draft_calls = 0, draft_offered = 0, draft_accepted = 0, draft_tail_steps = 0;

    // gitcap_distill (first use): the dual head's seven partials [slot 0's Mt][ntiles], both models' target logits
    // ([2][Mt])
    struct Distill { float *t_max = nullptr, *t_sum = nullptr, *s_max = nullptr, *s_sum = nullptr, *cross = nullptr, *rows = nullptr;
                     int *t_idx = nullptr, *s_idx = nullptr; } dist;

    // Frame window (gitcap_window_reset / _push / _greedy / _beam_search): the fp32 ln_post rows (no temporal embedding) of the
    // last win.slots frames of win_B clips, clip-major [B][F][N][Dv]; win (RingCursor) = where the next frame goes and how many
    // have been pushed.  win_order (RingOrder): a push orders itself behind the last window call's image prefix (it rewrites the
    // encoder workspace, hb included) and a window call behind the last push, whichever streams they were issued on.
    float* win_ring = nullptr;
    int64_t win_bytes = 0;
    int win_B = 0;
    RingCursor win;
    RingOrder win_order;

    // Stream pool (gitcap_pool_reset / _push / _greedy / _beam_search), allocated by pool_reset and state of its own beside the
    // window: pool_ring = the fp32 ln_post rows (no temporal embedding) of pool_S independent streams, [pool_S][F][N][Dv]; pool (one
    // RingCursor per stream) = where a stream's next frame goes and how many it holds.  pool_tab (device int32 [3][pool_cap]): the
    // ring frame of each packed frame of one push, then src / pos of each packed frame of one pool call (host_logic.h: pool_plan),
    // staged in pool_push_host / pool_call_host.  pool_order: win_order's discipline.
    float* pool_ring = nullptr;
    int32_t* pool_tab = nullptr;
    HostStage pool_push_host, pool_call_host;
    int pool_S = 0, pool_F = 0, pool_cap = 0;
    int64_t pool_bytes = 0;
    std::vector<RingCursor> pool;
    RingOrder pool_order;

    // instrumentation (bench.py): HIP-event brackets per kernel class, on the launch stream
    bool prof_on = false;
    struct ProfRec { hipEvent_t a, b; double flops, bytes; };
    struct ProfClass { std::vector<ProfRec> recs; size_t used = 0; };
    ProfClass prof[GITCAP_PROF_CLASSES];

    // gitcap_attention_map: the text pass slot 0 ran last on the caller's stream -- its rows, rows per clip and the positions
    // 0 .. T - 1 whose q | k the text cache holds (T == 0: none, or the image prefix changed since); permuted: a beam search or
    // gitcap_reorder_rows moved the rows.  stats: launch_attn_map's scratch for max rows x max_text_len, first use.
    struct AttnPass { int rows = 0, rows_per_clip = 0, T = 0; bool permuted = false; } att;
    float* att_stats = nullptr;
};

namespace {

// Number of decode streams the four slots share (slot i decodes on stream i % n).  HIP multiplexes streams onto
// GPU_MAX_HW_QUEUES (default 4) hardware queues; with one stream per slot the throughput depended on which streams
// happened to share a queue (1073-1723 captions/s over 1..8 queues, 1514 as soon as an RCCL communicator added its
// streams).  Two decode streams + the image-pass stream + the caller's stream fit the four queues: 1743 captions/s
// with or without RCCL.  One stream is too few: a token loop runs ~2x slower next to the GEMMs and must overlap
// another one to keep up with the image pass.
const int g_txt_streams = getenv("GITCAP_TXT_STREAMS") ? std::max(1, std::min(4, atoi(getenv("GITCAP_TXT_STREAMS")))) : 2;
// 256x256-tile count below which the 128x128 kernel is used (GITCAP_GEMM_SMALL_TILES=0 disables the switch)
std::atomic<int> g_small_tiles{getenv("GITCAP_GEMM_SMALL_TILES") ? atoi(getenv("GITCAP_GEMM_SMALL_TILES")) : 128};
// 128x128-tile count below which the 64x64 kernel is used (GITCAP_GEMM_TINY_TILES=0 disables the switch)
std::atomic<int> g_tiny_tiles{getenv("GITCAP_GEMM_TINY_TILES") ? atoi(getenv("GITCAP_GEMM_TINY_TILES")) : 200};     // measured crossover (tools/gemm_tiles_small.py): 180 -> 64x64, 228 -> 128x128

// (Until round 5 synchronous calls took 256(n) x 224(m) tiles -- a second tile kernel, gemm_mt.hip, 548 lines -- where that turned
// partial rounds on the 256 CUs into full ones: -1 ... -2 % per one-batch-at-a-time step, nothing for the pipelined path, whose idle
// CUs feed the token loops.  Retired in round 6: tools/experiments/gemm_mt.hip, profiles/r03_*, docs/LAB_NOTEBOOK.md.)
// polls a tile of a fused GEMM + LayerNorm launch spends waiting for its siblings before it gives up (0 = LN_SPIN_DEFAULT,
// ~30 s).  gitcap_dbg_config(6, n): a test forces the give-up path with n = 1.
std::atomic<unsigned> g_ln_spin_limit{0};

void select_slot(gitcap* h, int i) { h->cur_slot = i; }

// the stream pool's buffers (the caller has made sure nothing in flight uses them); pool_order's events stay for the next reset
void pool_free(gitcap* h) {
    if (h->pool_ring) (void)hipFree(h->pool_ring);
    if (h->pool_tab) (void)hipFree(h->pool_tab);
    h->pool_push_host.destroy();
    h->pool_call_host.destroy();
    h->pool_ring = nullptr;
    h->pool_tab = nullptr;
    h->pool_bytes = 0;
    h->pool_S = h->pool_F = h->pool_cap = 0;
    h->pool.clear();
}
gitcap::Slot& cur(gitcap* h) { return h->slots[h->cur_slot]; }      // the selected slot: every use of slot state goes through here

// Synchronous entry points (slot 0, caller's stream) share the image-row workspace with the submissions that
// gitcap_greedy_submit put on the handle's own streams: before a synchronous call touches it, the caller's stream
// waits for the token loop of every slot that has ever been submitted (each loop is ordered behind its image pass, so
// this covers the encoder stream too).  A wait on an event that has already fired costs nothing on the device.
hipError_t join_async(gitcap* h, hipStream_t stream) {
    if (h->next_ticket == 0) return hipSuccess;
    for (auto& sl : h->slots)
        if (sl.used) {
            hipError_t e = hipStreamWaitEvent(stream, sl.ev_dec, 0);
            if (e != hipSuccess) return e;
        }
    return hipSuccess;
}

// The statistics exchange of the fused GEMM + LayerNorm launches fails soft (gemm_epilogue.h): a tile that gave up waiting
// raised h->ln_fail.  Checked at every entry point that issues or joins device work and by gitcap_poll_errors: the device is
// drained, the word and the exchange barriers are reset, the handle stops using the fused epilogues (the GEMM + row-kernel
// form gives the same bits) and the caller is told once, so that it re-runs what it had in flight.
int poll_exchange(gitcap* h) {
    if (!h->ln_fail || !exchange_poll(h->xh, *(volatile unsigned*)h->ln_fail)) return 0;
    (void)hipDeviceSynchronize();
    h->poison_upto = poison_mark(h->next_ticket);   // every submission made so far may hold undefined rows: its wait says so, every time
    *(volatile unsigned*)h->ln_fail = 0;
    if (h->ln_cnt) (void)hipMemset(h->ln_cnt, 0, h->ln_cnt_words * sizeof(unsigned));
    h->win.clear();         // the frame window's rows may be undefined too: it is emptied, the caller pushes its frames again
    for (RingCursor& c : h->pool) c.reset(h->pool_F);       // and so is every stream of the pool
    return fail(h, GITCAP_ERR_EXCHANGE, "a GEMM + LayerNorm launch timed out waiting for its sibling tiles (CUs held by another "
                "process or a CU-masked stream?): results since the last call are undefined -- re-run them; this handle now uses "
                "separate LayerNorm launches");
}
#define POLL(h) do { int rc_ = poll_exchange(h); if (rc_) return rc_; } while (0)

struct ProfScope {
    gitcap* h; hipStream_t s; gitcap::ProfRec* r = nullptr;
    ProfScope(gitcap* h_, int cls, hipStream_t s_, double flops, double bytes) : h(h_), s(s_) {
        if (!h->prof_on) return;
        gitcap::ProfClass& pc = h->prof[cls];
        if (pc.used == pc.recs.size()) {
            gitcap::ProfRec n{};
            if (hipEventCreate(&n.a) != hipSuccess || hipEventCreate(&n.b) != hipSuccess) return;
            pc.recs.push_back(n);
        }
        r = &pc.recs[pc.used++];
        r->flops = flops; r->bytes = bytes;
        (void)hipEventRecord(r->a, s);
    }
    ~ProfScope() { if (r) (void)hipEventRecord(r->b, s); }
};

int ln(gitcap* h, hipStream_t s, const float* x, int ldx, const float* g, const float* b, float eps, int rows, int D,
       float* of, int ldf, bf16_t* ob, int ldb, const float* addv = nullptr, int add_div = 1, int add_mod = 1) {
    ProfScope ps(h, GITCAP_PROF_ROWOPS, s, 0.0, (double)rows * D * (4.0 + (of ? 4.0 : 0.0) + (ob ? 2.0 : 0.0)));
    LnArgs a{x, ldx, g, b, eps, rows, D, of, ldf, ob, ldb, addv, add_div, add_mod, nullptr, nullptr, 0.f};
    HIP_OK(h, launch_layernorm(a, s));
    return 0;
}

// Tile kernel selection.  a.M comes in as the valid rows of the launch padded to 256.  Few 256x256 tiles
// (small batches: one 6-frame clip is 5 x 3..12 tiles for 256 CUs) leave most of the chip idle: below g_small_tiles
// tiles the 128x128 kernel (4x the workgroups, two per CU) is used (B=1: 7.7 -> 6.8 ms per caption), and below
// g_tiny_tiles of THOSE the 64x64 kernel (16x, three per CU, 3-stage ring: the single-clip launches).  All tile kernels
// produce bitwise identical results (tests/test_kernels_gpu.py), so the choice only affects speed.
// Weights: bf16, or e4m3 bytes + row scales (W.scale != nullptr).  The tile kernels read e4m3 panels through bf16
// staging (a few MB: it stays in L2 / the Infinity Cache; HBM sees the e4m3 bytes): the four matrices of a transformer
// layer are expanded by ONE launch at the head of the layer (stage_layer), anything else right before its GEMM.
// Two alternatives were built in round 3 and measured slower at the configs[4] shape (bit-exact both): reading the bytes
// directly in the GEMM (LDS-DMA of the e4m3 panel, expansion on the fragment read, row scale on the accumulator): 10-25 %
// slower per launch, 32 v_cvt_scalef32_pk_bf16_fp8 per wave and K-tile next to 56-64 MFMAs
// (profiles/r03_gemm_e4m3_direct_vs_bf16.txt); expanding panel i+1 on a side stream while GEMM i runs (two-slot ring,
// events both ways): image pass 11.0 vs 10.3 ms, a cross-stream event hand-off costs more than the 3 us it hides.
// e4m3 storage: the bf16 panel a tile kernel reads for W -- the layer staging area when stage_layer expanded it, else the
// single-panel staging filled by a launch of its own, issued HERE (in front of the caller's ProfScope: a staging launch is
// not GEMM time).  bf16 storage: W itself.
hipError_t resolve_weight(gitcap* h, const WRef& W, int N, int K, hipStream_t s, const bf16_t** out) {
    *out = (const bf16_t*)W.p;
    if (!W.scale) return hipSuccess;
    for (int i = 0; i < h->n_staged; ++i)
        if (h->staged_src[i] == W.p) { *out = h->staged_dst[i]; return hipSuccess; }       // expanded at the head of the layer
    ProfScope ps(h, GITCAP_PROF_ROWOPS, s, 0.0, 3.0 * pad_to(N, 16) * (double)K);
    const hipError_t e = launch_dequant_fp8((const unsigned char*)W.p, W.scale, h->wstage, pad_to(N, 16), K, s);
    *out = h->wstage;
    return e;
}

hipError_t launch_gemm_auto(gitcap* h, GemmArgs a, int epi, hipStream_t s) {
    const bool ln = epi == EPI_RESID_LN_PRE || epi == EPI_RESID_LN_POST;
    if (ln) { a.ln_fail = h->ln_fail; a.ln_spin_limit = g_ln_spin_limit; }
    if (a.wscale) return launch_gemm256f8(a, epi, s);                 // e4m3 operands: one tile kernel, whatever the batch
    if (a.ln_out8 && ln) return launch_gemm256(a, epi, s);            // (its e4m3 LayerNorm copy: 256-row tiles only)
    if (gemm256_ok(a) && (a.M >> 8) * (a.N >> 8) >= g_small_tiles) return launch_gemm256(a, epi, s);
    if (ln) return hipErrorInvalidValue;
    if ((a.M & 63) == 0 && (a.N & 63) == 0 && ((a.M & 127) || (a.N & 127) || (a.M >> 7) * (a.N >> 7) < g_tiny_tiles))
        return launch_gemm64(a, epi, s);
    return launch_gemm(a, epi, s);
}

// e4m3 storage: expand the matrices of one transformer layer ([rows][K] each) into the layer staging area with ONE
// launch; the GEMMs of the layer then find them through staged_src.  Stream ordered: the previous layer's GEMMs (which read
// the area) are in front of this launch on the same stream.  No-op for bf16 storage.
int stage_layer(gitcap* h, hipStream_t s, const WRef* const* Ws, const int* rows, const int* Ks, int n) {
    h->n_staged = 0;
    if (n <= 0 || n > 4 || !Ws[0]->scale || !h->lstage) return 0;
    DequantBatch b{};
    size_t off = 0;
    for (int i = 0; i < n; ++i) {
        const size_t elems = (size_t)pad_to(rows[i], 16) * Ks[i];
        if (off + elems > h->lstage_elems) return fail(h, GITCAP_ERR_STATE, "stage_layer: staging area too small");
        b.w8[i] = (const unsigned char*)Ws[i]->p; b.scale[i] = Ws[i]->scale; b.out[i] = h->lstage + off; b.K[i] = Ks[i];
        b.n16[i] = (int64_t)(elems / 16);
        h->staged_src[i] = Ws[i]->p; h->staged_dst[i] = h->lstage + off;
        off += elems;
    }
    b.n = n;
    HIP_OK(h, launch_dequant_fp8_batch(b, s));
    h->n_staged = n;
    return 0;
}

// `rows` = the valid rows (M = rows padded to 256): the algorithmic work of the bracket and what the tile choice is made on
int gemm(gitcap* h, hipStream_t s, int epi, const bf16_t* A, int lda, const WRef& W, const float* bias, int rows, int M, int N,
         int K, void* out, int ldo, const float* resid = nullptr, int ldr = 0) {
    GemmArgs a{};
    HIP_OK(h, resolve_weight(h, W, N, K, s, &a.W));
    // algorithmic work: the VALID rows, not the padded M that is launched; bytes = operands once + the output (+ the fp32
    // residual read)
    const double R = rows, osz = (epi == EPI_BIAS_RESID_F32 || epi == EPI_BIAS_F32 || epi == EPI_PATCH_F32) ? 4.0 : 2.0;
    ProfScope ps(h, GITCAP_PROF_GEMM, s, 2.0 * R * N * K, 2.0 * R * K + 2.0 * N * K + R * N * (osz + (resid ? 4.0 : 0.0)));
    a.A = A; a.lda = lda; a.bias = bias; a.M = M; a.N = N; a.K = K; a.out = out; a.ldo = ldo;
    a.resid = resid; a.ldr = ldr;
    HIP_OK(h, launch_gemm_auto(h, a, epi, s));
    return 0;
}

std::atomic<bool> g_fuse_ln{!env_flag("GITCAP_NO_GEMM_LN")};

// compute = fp8_ffn: FC1 and FC2 of the image rows on v_mfma_f32_16x16x128_f8f6f4 (gemm256.hip).  Their activation operands
// (the LayerNorm output in front of FC1, the GELU output in front of FC2) are written as e4m3 codes of value / f8_scale by the
// producing epilogues -- one static power-of-two scale per handle (default 1/16: codes cover +-28), saturating, every clamped
// code of a valid row counted (gitcap_fp8_saturations) --, the weights are the e4m3 codes of
// e4m3 storage read as they are.  Everything else (q|k|v, attention, output projections, the text rows) stays bf16.  The e4m3
// copy of a LayerNorm output exists only in the fused GEMM + LayerNorm epilogue, so the mode needs it (a handle whose exchange
// timed out computes in bf16 from then on).
bool use_f8(const gitcap* h) { return h->f8ffn && g_fuse_ln && !h->xh.degraded; }

// FC1 of the image rows in fp8 compute: A8 = e4m3 codes [M][K] (value / f8_scale), W = e4m3 storage; out8 = e4m3 codes of
// GELU(A W^T + bias) / f8_scale
int gemm_f8(gitcap* h, hipStream_t s, int epi, const unsigned char* A8, int lda, const WRef& W, const float* bias, int rows,
            int M, int N, int K, unsigned char* out8, int ldo) {
    if (!W.scale) return fail(h, GITCAP_ERR_STATE, "fp8 compute needs e4m3 weight storage");
    ProfScope ps(h, GITCAP_PROF_GEMM, s, 2.0 * rows * N * K, 1.0 * rows * K + 1.0 * N * K + 1.0 * rows * N);
    GemmArgs a{};
    a.A = (const bf16_t*)A8; a.lda = lda; a.W = (const bf16_t*)W.p; a.wscale = W.scale; a.ascale = h->f8_scale; a.bias = bias;
    a.M = M; a.N = N; a.K = K; a.out = out8; a.ldo = ldo; a.out8_inv = 1.0f / h->f8_scale;
    a.valid_rows = rows; a.f8_sat = h->f8_sat;
    HIP_OK(h, launch_gemm_auto(h, a, epi, s));
    return 0;
}

// what a caller of gemm_ln may ask for beyond the plain form
struct LnOpts {
    const float* addv = nullptr;    // nullable: LayerNorm output += addv[((row / add_div) % add_mod) * N + n] (temporal embedding)
    int add_div = 1, add_mod = 1;
    float* ln_f32 = nullptr;        // nullable: the LayerNorm output in fp32 as well
    // ln8 (fp8 compute): also write the LayerNorm output as e4m3 codes (the next FC1's operand).  f8in: A is e4m3 codes
    // [M][lda bytes] and W the e4m3 storage (FC2 in fp8 compute).  Both exist in the fused epilogue only.
    unsigned char* ln8 = nullptr;
    bool f8in = false;
};

// GEMM (+ bias [+ residual]) followed by LayerNorm of its output rows.
//   post = false (pre-LN ViT block):   x = A W^T + bias + resid -> xout (fp32, may alias resid);  ln_b = bf16 LN(x)
//   post = true  (post-LN decoder):    x = A W^T + bias [+ resid] -> scratch; xout = fp32 LN(x) (may alias resid); ln_b = bf16 LN(x)
// Large launches run both inside the 256x256 kernel (EPI_RESID_LN_*: the tiles of a row block exchange segment
// statistics); small ones the 128x128 kernel + the row kernel.  Both give the same bits (ln_canon.h).
// GITCAP_NO_GEMM_LN=1 (diagnosis / A-B only) keeps every LayerNorm a launch of its own; so does a handle whose exchange
// ever timed out (poll_exchange).
int gemm_ln(gitcap* h, hipStream_t s, bool post, const bf16_t* A, int lda, const WRef& W, const float* bias, int M, int N,
            int K, float* xout, const float* resid, const float* ln_g, const float* ln_b, float eps, int rows,
            bf16_t* ln_out, float* scratch, const LnOpts& o = {}) {
    const float* const addv = o.addv; const int add_div = o.add_div, add_mod = o.add_mod;
    float* const ln_f32 = o.ln_f32; unsigned char* const ln8 = o.ln8; const bool f8in = o.f8in;
    GemmArgs a{};
    a.A = A; a.lda = lda; a.bias = bias; a.M = M; a.N = N; a.K = K; a.out = xout; a.ldo = N; a.resid = resid; a.ldr = N;
    a.ln_out8 = ln8; a.ld_ln8 = N; a.ln_out8_inv = 1.0f / h->f8_scale; a.f8_sat = h->f8_sat;
    if (f8in) { a.W = (const bf16_t*)W.p; a.wscale = W.scale; a.ascale = h->f8_scale; }
    const bool force_fused = ln8 != nullptr || f8in;
    // the e4m3 LayerNorm copy of the fp8-operand kernel exists for the PRE form only (gemm256.hip: gemm256f8_kernel, LN8 = EPI_RESID_LN_PRE)
    if (f8in && ln8 && post) return fail(h, GITCAP_ERR_STATE, "fp8 compute: no e4m3 LayerNorm copy in the post-LN form of the fp8-operand GEMM");
    a.ln_g = ln_g; a.ln_b = ln_b; a.ln_eps = eps; a.ln_out = ln_out; a.ld_ln = N; a.ln_stats = h->ln_stats; a.ln_cnt = h->ln_cnt;
    a.ln_stats_rows = h->Mi;
    a.ln_add = addv; a.ln_add_div = add_div; a.ln_add_mod = add_mod; a.ln_out_f32 = ln_f32; a.ld_ln_f32 = N; a.valid_rows = rows;
    // ln_out may be the A operand itself (visual projection): a tile writes its rows only after every tile that reads
    // them has finished its K loop (that is what the exchange waits for) -- as long as both views have the same row stride
    const bool alias_ok = (const void*)A != (const void*)ln_out || lda == N;
    if (force_fused && !(g_fuse_ln && !h->xh.degraded && alias_ok && gemm256_ln_ok(a) && (post ? (xout && !addv && !ln_f32) : resid != nullptr)))
        return fail(h, GITCAP_ERR_STATE, "fp8 compute: a GEMM + LayerNorm launch cannot take the fused epilogue");
    if (g_fuse_ln && !h->xh.degraded && alias_ok && gemm256_ln_ok(a) && (force_fused || (M >> 8) * (N >> 8) >= g_small_tiles) &&
        (post ? (xout && !addv && !ln_f32) : resid != nullptr)) {
        if (!f8in) HIP_OK(h, resolve_weight(h, W, N, K, s, &a.W));
        const double R = rows, esz = f8in ? 1.0 : 2.0;   // A + W + fp32 out + bf16 LayerNorm out (+ fp32 residual read)
        ProfScope ps(h, GITCAP_PROF_GEMM_LN, s, 2.0 * R * N * K, esz * R * K + esz * N * K + R * N * ((xout ? 4.0 : 0.0) + 2.0 + (ln_f32 ? 4.0 : 0.0) + (resid ? 4.0 : 0.0)));
        HIP_OK(h, launch_gemm_auto(h, a, post ? EPI_RESID_LN_POST : EPI_RESID_LN_PRE, s));
        return 0;
    }
    int rc;
    // GEMM, then the row kernel: x goes to the scratch (post), to xout, or -- when the caller does not want it -- over the residual
    float* xo = post ? scratch : (xout ? xout : const_cast<float*>(resid));
    if ((rc = gemm(h, s, resid ? EPI_BIAS_RESID_F32 : EPI_BIAS_F32, A, lda, W, bias, rows, M, N, K, xo, N, resid, N))) return rc;
    return ln(h, s, xo, N, ln_g, ln_b, eps, rows, N, post ? xout : ln_f32, N, ln_out, N, addv, add_div, add_mod);
}

int skinny(gitcap* h, hipStream_t s, int epi, const bf16_t* X, int ldx, const WRef& W, const float* bias, int M,
           int N, int K, void* out, int ldo, int T = 1, int row_stride = 1, int row_off = 0) {
    ProfScope ps(h, GITCAP_PROF_SKINNY, s, 2.0 * M * N * K, (W.scale ? 1.0 : 2.0) * N * K);
    SkinnyArgs a{X, ldx, W.p, W.scale, bias, M, N, K, out, ldo, T, row_stride, row_off, nullptr, nullptr};
    a.Wpk = W.pk;
    HIP_OK(h, launch_skinny(a, epi, s));
    return 0;
}

int skinny_splitk(gitcap* h, hipStream_t s, const bf16_t* X, int ldx, const WRef& W, int M, int N, int K, float* slabs, int ksplit = 0) {
    ProfScope ps(h, GITCAP_PROF_SKINNY, s, 2.0 * M * N * K, (W.scale ? 1.0 : 2.0) * N * K);
    SkinnyArgs a{X, ldx, W.p, W.scale, nullptr, M, N, K, slabs, N, 1, 1, 0, nullptr, nullptr};
    a.Wpk = W.pk; a.ksplit = ksplit;
    HIP_OK(h, launch_skinny_splitk(a, s));
    return 0;
}

int ln_reduce(gitcap* h, hipStream_t s, const float* slabs, int nslab, const float* bias, const float* resid,
              const float* g, const float* b, float eps, int M, int D, float* xf, bf16_t* xb) {
    ProfScope ps(h, GITCAP_PROF_SKINNY, s, 0.0, (double)M * D * (4.0 * nslab + 4.0 + 6.0));   // text-path class
    HIP_OK(h, launch_ln_reduce(slabs, nslab, bias, resid, g, b, eps, M, D, xf, xb, s));
    return 0;
}

// projected image tokens -> decoder layers over image rows only; fills kv_img (text independent)
// ragged_rows > 0 (a ragged batch, h->call.fc its counts): the packed rows of B clips whose tables the slot's off / len hold, S the
// longest clip's -- every GEMM and row kernel sees the ragged_rows valid rows, the attention runs its variable-length form
int image_prefix(gitcap* h, int B, int S, hipStream_t s, int ragged_rows = 0) {
    const gitcap_config& c = h->c;
    gitcap::Slot& sl = cur(h);
    const bool ragged = ragged_rows > 0;
    const int D = h->D, Dv = h->Dv, rows = ragged ? ragged_rows : B * S, Mp = pad_to(rows, 256);
    double attn_pairs = (double)B * S * S;                   // (query, key) pairs per head
    if (ragged) {
        attn_pairs = 0.0;
        for (int b = 0; b < h->call.fc.B; ++b) attn_pairs += (double)h->call.fc.n[b] * h->N * h->call.fc.n[b] * h->N;
    }
    int rc;
    h->n_staged = 0;
    // 'linearLn' projection: Linear(Dv -> D) + LayerNorm
    if ((rc = gemm_ln(h, s, true, h->hb, Dv, h->vproj_w, h->vproj_b, Mp, D, Dv, h->x, nullptr, h->vproj_lnw, h->vproj_lnb,
                      c.proj_ln_eps, rows, h->hb, h->tmp))) return rc;
    const size_t kv_layer = (size_t)h->Mi * 3 * D;
    const bool f8 = use_f8(h);
    const bool hid = h->want_hidden && h->cur_slot == 0 && !h->pipelined;     // hidden-state export: synchronous path only
    auto keep = [&](int entry) -> hipError_t {
        return hid ? hipMemcpyAsync(h->hid_img + (size_t)entry * h->Mi * D, h->x, (size_t)rows * D * 4, hipMemcpyDeviceToDevice, s) : hipSuccess;
    };
    HIP_OK(h, keep(0));
    // kv_cache = v_e4m3: the text attention's copy of this layer's V rows (codes + scales); the image rows' own attention keeps bf16
    auto quant_v = [&](int l, const bf16_t* kv) -> int {
        if (!h->kv_v8) return 0;
        ProfScope ps(h, GITCAP_PROF_ROWOPS, s, 0.0, (double)rows * D * 3.0);
        HIP_OK(h, launch_kv_quant_v(kv, sl.v8_img + (size_t)l * h->Mi * D, sl.vs_img + (size_t)l * h->Mi * c.dec_heads, rows, D, c.dec_heads, h->Mi, s));
        return 0;
    };
    for (int l = 0; l < c.dec_layers; ++l) {
        const DecLayer& L = h->dec[l];
        bf16_t* kv = sl.kv_img + (size_t)l * kv_layer;
        if (l + 1 < c.dec_layers || hid) {
            {   // e4m3 storage: the layer's matrices -> bf16 staging, one launch (fp8 compute reads FC1 / FC2 as they are)
                const WRef* ws[4] = {&L.qkvw, &L.aow, &L.fc1w, &L.fc2w};
                const int wr[4] = {3 * D, D, c.dec_ffn, D}, wk[4] = {D, D, D, c.dec_ffn};
                if ((rc = stage_layer(h, s, ws, wr, wk, f8 ? 2 : 4))) return rc;
            }
            if ((rc = gemm(h, s, EPI_BIAS_BF16, h->hb, D, L.qkvw, L.qkvb, rows, Mp, 3 * D, D, kv, 3 * D))) return rc;
            if ((rc = quant_v(l, kv))) return rc;
            {
                ProfScope ps(h, GITCAP_PROF_ATTN_FULL, s, 4.0 * c.dec_heads * attn_pairs * 64, 0.0);
                if (ragged) HIP_OK(h, launch_attn_full_varlen(kv, h->ctx, B, sl.off, sl.len, S, c.dec_heads, s));
                else HIP_OK(h, launch_attn_full(kv, h->ctx, B, S, c.dec_heads, s));
            }
            LnOpts ao; ao.ln8 = f8 ? h->hb8 : nullptr;
            if ((rc = gemm_ln(h, s, true, h->ctx, D, L.aow, L.aob, Mp, D, D, h->x, h->x, L.ln1w, L.ln1b, c.dec_ln_eps, rows,
                              h->hb, h->tmp, ao))) return rc;
            if (f8) rc = gemm_f8(h, s, EPI_BIAS_GELU_F8, h->hb8, D, L.fc1w, L.fc1b, rows, Mp, c.dec_ffn, D, h->ffn8, c.dec_ffn);
            else rc = gemm(h, s, EPI_BIAS_GELU_BF16, h->hb, D, L.fc1w, L.fc1b, rows, Mp, c.dec_ffn, D, h->ffn, c.dec_ffn);
            if (rc) return rc;
            LnOpts fc2; fc2.f8in = f8;
            if ((rc = gemm_ln(h, s, true, f8 ? (const bf16_t*)h->ffn8 : h->ffn, c.dec_ffn, L.fc2w, L.fc2b, Mp, D, c.dec_ffn, h->x, h->x, L.ln2w, L.ln2b,
                              c.dec_ln_eps, rows, h->hb, h->tmp, fc2))) return rc;
            HIP_OK(h, keep(l + 1));
        } else {
            // last layer: image rows are only ever read as keys/values -> K,V projections only
            if ((rc = gemm(h, s, EPI_BIAS_BF16, h->hb, D, L.qkvw.rows_from(D, D), L.qkvb + D, rows, Mp, 2 * D, D, kv + D, 3 * D))) return rc;
            if ((rc = quant_v(l, kv))) return rc;
        }
    }
    sl.B = B; sl.S = S; sl.S_tot = rows; sl.ragged = ragged; sl.have = true;
    if (h->cur_slot == 0) h->att = gitcap::AttnPass{};      // the cached text rows were computed against another image prefix
    return 0;
}

// The greedy loop chains token steps: `pre_embedded` = the input rows of this step (embedding of the token at position t0 +
// LayerNorm) were already produced by the previous step's arg-max launch; `embed_next` = this step's arg-max launch produces
// the next step's.  Same row code either way (rowln.h); one launch less per token step.  Only with more than two rows (with
// one or two the q|k|v launch embeds its rows itself) and one position per row.
std::atomic<bool> g_chain_steps{!env_flag("GITCAP_NO_STEP_CHAIN")};       // gitcap_dbg_config(5, .)
// fragment-major copies of the text-path weights, made by gitcap_finalize_weights (GITCAP_NO_WPACK / gitcap_dbg_config(8, 0):
// the kernels read the row-major originals; same bits, slower; the FFN then runs as two launches)
std::atomic<bool> g_wpack{!env_flag("GITCAP_NO_WPACK")};
std::atomic<bool> g_ffn_fuse{!env_flag("GITCAP_NO_FFN_FUSE")};            // gitcap_dbg_config(7, .): ffn_txt.hip vs FC1 + split-K FC2 launches

bool text_chain_ok(gitcap* h, int rows, int T) {
    return g_chain_steps && T == 1 && !(h->want_hidden && h->cur_slot == 0 && !h->pipelined) &&
           !(g_row_prologue && skinny_row_prologue_ok(rows, h->D, h->dec[0].qkvw.scale != nullptr));
}

// A pass of the decoder over text rows (RowsReq, kernels.h) and what only this stack takes: rows = clips * beams; all_positions:
// logits of every position instead of the last; the per-step modifiers pre_embedded / embed_next (above) and ban (the BAN form of the head, nullable).  keep_len (nullable): the KEEP form of the arg-max launch.
// verify (a draft's verify pass): the head over ALL rows x T positions, arg-max partials only (+ the sum partial: verify_lp), no
// logits and no arg-max launch -- launch_draft_accept_rows reduces them.
struct TextReq : RowsReq {
    int beams = 1, all_positions = 0;
    bool pre_embedded = false, embed_next = false;
    const HeadBan* ban = nullptr;
    const int32_t* keep_len = nullptr;
    bool verify = false, verify_lp = false;
};

int text_forward(gitcap* h, const TextReq& q, hipStream_t s) {
    const gitcap_config& c = h->c;
    const int64_t* const ids = q.ids;
    const int ld_ids = q.ld_ids, rows = q.rows, beams = q.beams, t0 = q.t0, T = q.T;
    gitcap::Slot& sl = cur(h);
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "weights not finalized");
    if (!sl.have) return fail(h, GITCAP_ERR_STATE, "text_forward before encode/set_visual");
    if (!ids || rows <= 0 || beams <= 0 || T <= 0 || t0 < 0) return fail(h, GITCAP_ERR_ARG, "text_forward: bad arguments");
    if (rows != sl.B * beams) return fail(h, GITCAP_ERR_ARG, "text_forward: rows != encoded clips * beams");
    if (rows > h->R) return fail(h, GITCAP_ERR_ARG, "text_forward: rows exceed max_batch*max_beams");
    if (t0 + T > h->Tmax) return fail(h, GITCAP_ERR_ARG, "text_forward: t0+T exceeds max_text_len");
    if (t0 + T > c.max_text_pos) return fail(h, GITCAP_ERR_ARG, "text_forward: position exceeds max_text_pos");
    const int D = h->D, M = rows * T, H = c.dec_heads;
    if (M > sl.Mt) return fail(h, GITCAP_ERR_STATE, "text_forward: more text rows than the slot's workspace holds");
    if (h->cur_slot == 0) {     // what gitcap_attention_map may read back: a synchronous pass from position 0, and the steps that extend it
        gitcap::AttnPass& ap = h->att;
        if (h->pipelined) ap = gitcap::AttnPass{};
        else if (t0 == 0) ap = gitcap::AttnPass{rows, beams, T, false};
        else if (ap.rows == rows && ap.rows_per_clip == beams && t0 <= ap.T) ap.T = t0 + T;
        else ap = gitcap::AttnPass{};
    }
    int rc;
    const size_t kvi_layer = (size_t)h->Mi * 3 * D, kvt_layer = (size_t)h->R * h->Tmax * 3 * D;
    // FC1 -> GELU -> FC2 of the text rows: one launch over 64-wide hidden slices (ffn_txt.hip), leaving dec_ffn / 64 fp32
    // slabs; or (GITCAP_NO_FFN_FUSE / gitcap_dbg_config(7, 0): A-B and cross-check) the FC1 launch + the split-K FC2 launch
    // over the same slabs -- the same bits either way
    const bool ffn_slices = ffn_txt_ok(D, c.dec_ffn) && c.dec_ffn / 64 <= h->nslab_max;
    const bool ffn_fused = ffn_slices && g_ffn_fuse && h->dec[0].fc1w.pk && h->dec[0].fc2w.pk;
    const int ks_f = ffn_slices ? c.dec_ffn / 64 : skinny_ksplit(c.dec_ffn);
    const bool hid = h->want_hidden && h->cur_slot == 0 && !h->pipelined && t0 == 0;    // hidden-state export: a whole prefix, synchronous path
    auto keep_txt = [&](int entry) -> hipError_t {                       // xs = the text rows' input of layer `entry`
        return hid ? hipMemcpyAsync(h->hid_txt + (size_t)entry * h->Mt * D, sl.xs, (size_t)M * D * 4, hipMemcpyDeviceToDevice, s) : hipSuccess;
    };
    if (hid) h->hid_T = T;
    // Per layer 5 launches: [text embedding | reduce of the previous layer's FC2 slabs + LayerNorm], q|k|v projection
    // straight into the text K/V cache, attention + output dense + LayerNorm (txtblock.hip), FC1 + GELU, FC2 as split-K
    // partial slabs.  With one or two rows (a single clip: the webcam case) the first of the five runs inside the second
    // (skinny.hip "row prologue": every workgroup of the q|k|v launch computes the rows itself): 4 launches per layer.
    // The residual rows then alternate between two buffers (workgroup 0 writes them while the others still read the old).
    const bool rows_pro = g_row_prologue && !hid && skinny_row_prologue_ok(M, D, h->dec[0].qkvw.scale != nullptr);
    float *xcur = sl.xs, *xalt = sl.xs2;
    for (int l = 0; l < c.dec_layers; ++l) {
        const DecLayer& L = h->dec[l];
        bf16_t* kvt = sl.kv_txt + (size_t)l * kvt_layer;
        if (rows_pro) {
            ProfScope ps(h, GITCAP_PROF_SKINNY, s, 2.0 * M * 3 * D * D, 2.0 * 3 * D * D);
            SkinnyArgs a{sl.xsb, D, L.qkvw.p, nullptr, L.qkvb, M, 3 * D, D, kvt, 3 * D, T, h->Tmax, t0, nullptr, nullptr};
            a.Wpk = L.qkvw.pk;
            if (l == 0) {
                a.ln.kind = 2; a.ln.ids = ids; a.ln.ld_ids = ld_ids; a.ln.T = T; a.ln.t0 = t0; a.ln.vocab = c.vocab_size;
                a.ln.word = h->word; a.ln.pos = h->tpos; a.ln.g = h->txt_lnw; a.ln.b = h->txt_lnb;
            } else {
                const DecLayer& P = h->dec[l - 1];
                a.ln.kind = 1; a.ln.slabs = sl.slabs; a.ln.nslab = ks_f; a.ln.bias = P.fc2b; a.ln.resid = xcur; a.ln.g = P.ln2w; a.ln.b = P.ln2b;
            }
            a.ln.eps = c.dec_ln_eps; a.ln.xf = xalt;
            HIP_OK(h, launch_skinny(a, SK_BIAS_BF16, s));
            std::swap(xcur, xalt);
        } else {
            if (l == 0) {
                if (!q.pre_embedded)
                    HIP_OK(h, launch_embed_text(ids, ld_ids, rows, T, t0, h->word, h->tpos, h->txt_lnw, h->txt_lnb, c.dec_ln_eps, D,
                                                c.vocab_size, xcur, sl.xsb, s));
            } else {
                const DecLayer& P = h->dec[l - 1];
                if ((rc = ln_reduce(h, s, sl.slabs, ks_f, P.fc2b, xcur, P.ln2w, P.ln2b, c.dec_ln_eps, M, D, xcur, sl.xsb))) return rc;
            }
            HIP_OK(h, keep_txt(l));
            if ((rc = skinny(h, s, SK_BIAS_BF16, sl.xsb, D, L.qkvw, L.qkvb, M, 3 * D, D, kvt, 3 * D, T, h->Tmax, t0))) return rc;
        }
        {
            TxtBlockArgs ta{};
            ta.kv_img = sl.kv_img + (size_t)l * kvi_layer; ta.kv_txt = kvt;
            ta.rows = rows; ta.beams = beams; ta.t0 = t0; ta.T = T; ta.Tmax = h->Tmax; ta.S_img = sl.S; ta.H = H; ta.D = D;
            ta.aow = L.aow.p; ta.aowpk = L.aow.scale ? nullptr : L.aow.pk; ta.aoscale = L.aow.scale; ta.aob = L.aob; ta.g1 = L.ln1w; ta.b1 = L.ln1b; ta.xin = xcur; ta.eps = c.dec_ln_eps;
            ta.part = sl.part; ta.cnt = sl.row_cnt; ta.xs = xcur; ta.xsb = sl.xsb;
            if (h->kv_v8) { ta.v8_img = sl.v8_img + (size_t)l * h->Mi * D; ta.vs_img = sl.vs_img + (size_t)l * h->Mi * H; ta.v8_pitch = h->Mi; }
            // K/V of all layers that one token step streams: beyond what the 256 MiB Infinity Cache can keep next to the
            // 132 MB of decoder weights, the rows are loaded non-temporally (16 clips x 6 frames: 349 MB per step; measured
            // +0.6 % pipelined, -1 % serial step; one clip stays cached across steps and is 4 % faster with the default policy)
            // (S_tot = the image rows of all clips, B * S of a dense prefix; every beam of a clip streams its clip's rows)
            ta.nt_kv = (double)sl.S_tot * c.dec_layers * 2.0 * D * 2.0 > 128e6 ? 1 : 0;
            if (sl.ragged) { ta.off = sl.off; ta.len = sl.len; }
            double kvb = 0;
            for (int j = 0; j < T; ++j) kvb += ((double)beams * sl.S_tot + (double)rows * (t0 + j + 1)) * 2 * D * 2;
            if (h->kv_v8) kvb -= (double)beams * T * sl.S_tot * (D - 4.0 * H);     // image V: 1 byte per element + 4 per (key, head)
            ProfScope ps(h, GITCAP_PROF_ATTN_TEXT, s, 0.0, kvb + (L.aow.scale ? 1.0 : 2.0) * D * D);     // K/V read once + the output dense
            HIP_OK(h, launch_txt_block(ta, s));
        }
        if (ffn_fused) {
            ProfScope ps(h, GITCAP_PROF_SKINNY, s, 4.0 * M * c.dec_ffn * D, (L.fc1w.scale ? 1.0 : 2.0) * 2.0 * c.dec_ffn * D);
            FfnTxtArgs fa{sl.xsb, D, L.fc1w.pk, L.fc2w.pk, L.fc1w.scale, L.fc2w.scale, L.fc1b, M, D, c.dec_ffn, sl.slabs};
            HIP_OK(h, launch_ffn_txt(fa, s));
        } else {
            if ((rc = skinny(h, s, SK_BIAS_GELU_BF16, sl.xsb, D, L.fc1w, L.fc1b, M, c.dec_ffn, D, sl.fs, c.dec_ffn))) return rc;
            if ((rc = skinny_splitk(h, s, sl.fs, c.dec_ffn, L.fc2w, M, D, c.dec_ffn, sl.slabs, ffn_slices ? ks_f : 0))) return rc;
        }
    }
    {   // the last layer's FC2 reduce + bias + residual + LayerNorm
        const DecLayer& P = h->dec[c.dec_layers - 1];
        if ((rc = ln_reduce(h, s, sl.slabs, ks_f, P.fc2b, xcur, P.ln2w, P.ln2b, c.dec_ln_eps, M, D, xcur, sl.xsb))) return rc;
        HIP_OK(h, keep_txt(c.dec_layers));
    }
    if (!q.logits_out && !q.argmax_out && !q.score && !q.verify) return 0;
    // vocabulary head (+ arg-max partials per 16-column tile, reduced by argmax_final)
    const int V = c.vocab_size, ntiles = (V + 15) / 16;
    if (q.verify) {     // gitcap_greedy_draft: the partials of all positions, what the token steps' heads would have left one by one
        if (q.verify_lp && !sl.amax_sum) return fail(h, GITCAP_ERR_STATE, "text_forward: token log-probabilities without their partials");
        SkinnyArgs va;
        vocab_head_args(va, HeadWeight{h->head_w.p, h->head_w.pk, h->head_w.scale, h->head_b, V, D}, sl.xsb, rows, T, true, nullptr,
                        sl.amax_val, sl.amax_idx, q.verify_lp ? sl.amax_sum : nullptr);
        ProfScope ps(h, GITCAP_PROF_SKINNY, s, 2.0 * va.M * V * D, (va.wscale ? 1.0 : 2.0) * V * D);
        HIP_OK(h, launch_skinny(va, SK_BIAS_F32, s));
        return 0;
    }
    if (q.score) {      // gitcap_score: all positions, no logits; the three partials + the given tokens' logits -> score_final
        if (!sl.amax_sum || !sl.score_buf) return fail(h, GITCAP_ERR_STATE, "text_forward: scoring without its buffers");
        ProfScope ps(h, GITCAP_PROF_SKINNY, s, 2.0 * M * V * D, (h->head_w.scale ? 1.0 : 2.0) * V * D);
        HIP_OK(h, launch_score(HeadWeight{h->head_w.p, h->head_w.pk, h->head_w.scale, h->head_b, V, D}, sl.xsb, ids, ld_ids, rows, T,
                               sl.amax_val, sl.amax_idx, sl.amax_sum, sl.score_buf, *q.score, s));
        return 0;
    }
    if ((q.lp_out || q.topk.k) && (!q.argmax_out || !sl.amax_sum))
        return fail(h, GITCAP_ERR_STATE, "text_forward: token log-probabilities or top-k alternatives without their partials");
    SkinnyArgs ha;      // amax_sum: the head's third partial -> the chosen token's log-probability (argmax_final), the alternatives' (head_topk)
    const HeadWeight hw{h->head_w.p, h->head_w.pk, h->head_w.scale, h->head_b, V, D};
    const HeadRows hr = vocab_head_args(ha, hw, sl.xsb, rows, T, q.all_positions && q.logits_out, q.logits_out,
                                        q.argmax_out ? sl.amax_val : nullptr, q.argmax_out ? sl.amax_idx : nullptr,
                                        q.lp_out || q.topk.k ? sl.amax_sum : nullptr);
    {
        ProfScope ps(h, GITCAP_PROF_SKINNY, s, 2.0 * ha.M * V * D, (ha.wscale ? 1.0 : 2.0) * V * D);
        HIP_OK(h, launch_skinny(ha, SK_BIAS_F32, s, nullptr, q.ban));     // ban (constrained greedy step): the BAN form of the head
    }
    // the model's own k best of the same row, whatever a prompt forces into the position: AHEAD of the arg-max launch, which may
    // embed the next step's input rows over the head's (embed_next writes sl.xsb)
    if (q.topk.k) {
        HeadTopkArgs ta{};
        ta.X = ha.X; ta.ldx = ha.ldx; ta.hw = hw; ta.val = sl.amax_val; ta.idx = sl.amax_idx; ta.sum = sl.amax_sum; ta.bn = q.ban;
        ta.rows = rows; ta.T = 1; ta.row_stride = hr.am_stride; ta.row_off = hr.am_off;
        ta.k = q.topk.k; ta.top_ids = q.topk.ids; ta.top_lp = q.topk.lp; ta.ld = q.topk.ld;
        ProfScope ps(h, GITCAP_PROF_SKINNY, s, 2.0 * rows * q.topk.k * 16 * D, (hw.wscale ? 1.0 : 2.0) * rows * q.topk.k * 16 * D);
        HIP_OK(h, launch_head_topk(ta, s));
    }
    if (q.argmax_out) {
        const NextEmbed ne{h->word, h->tpos, h->txt_lnw, h->txt_lnb, c.dec_ln_eps, D, c.vocab_size, t0 + 1, sl.xs, sl.xsb};
        ArgmaxArgs a{};
        a.val = sl.amax_val; a.idx = sl.amax_idx; a.sum = q.lp_out ? sl.amax_sum : nullptr; a.ntiles = ntiles;
        a.rows = rows; a.row_stride = hr.am_stride; a.row_off = hr.am_off;
        a.out = q.argmax_out; a.ld_out = q.ld_argmax; a.sep_cnt = q.sep_cnt; a.step = q.step; a.sep_id = c.sep_token_id;
        a.lp_out = q.lp_out; a.ld_lp = q.ld_lp; a.emb = q.embed_next ? &ne : nullptr;
        a.prompt = q.prompt; a.prompt_pos = t0 + T;       // (greedy loop): the token goes to position t0 + T, where a row's prompt may still stand
        a.keep_len = q.keep_len;                          // (a draft's tail): or the row's verified part
        HIP_OK(h, launch_argmax_final(a, s));
    }
    return 0;
}

int check_frames(gitcap* h, const void* frames, int B, int F, bool raw = false) {
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "weights not finalized");
    if (!frames || B <= 0 || F <= 0) return fail(h, GITCAP_ERR_ARG, "encode: bad arguments");
    if (B > h->c.max_batch || F > h->c.max_frames) return fail(h, GITCAP_ERR_ARG, "encode: B/F exceed the sizes the handle was created for");
    if (h->c.num_frames > 0 && F > h->c.num_frames) return fail(h, GITCAP_ERR_ARG, "encode: more frames than temporal embeddings");
    if (!raw && ((uintptr_t)frames & 15) != 0) return fail(h, GITCAP_ERR_ARG, "encode: frames must be 16-byte aligned");
    return 0;
}

int check_raw(gitcap* h, const uint8_t* frames, int B, int F, int H, int W) {
    if (!frames || H <= 0 || W <= 0) return fail(h, GITCAP_ERR_ARG, "raw frames: null pointer or empty frames");
    if ((int64_t)B * F * H * W * 3 > ((int64_t)1 << 40)) return fail(h, GITCAP_ERR_ARG, "raw frames: sizes overflow");
    return check_frames(h, frames, B, F, true);
}

}  // namespace

struct FrameSrc { const float* f32; const uint8_t* u8; int H, W; };     // fp32 NCHW (CLIP-normalised) or raw uint8 HWC BGR
static int encode_impl(gitcap* h, FrameSrc src, int B, int F, float* visual_out, hipStream_t stream);
static int encode_sync(gitcap* h, FrameSrc src, int B, int F, float* visual_out, hipStream_t s);

// What the entry points take of the pending attachments (CallScope, host_logic.h): taken parts are consumed whatever becomes of
// the call; a call without an image pass of its own frames refuses frame counts (REFUSE_FC: cleared, and the call fails).
constexpr unsigned TAKE_GREEDY = OPT_LP | OPT_PR | OPT_CO | OPT_TK, TAKE_BEAM = OPT_SO | OPT_PR | OPT_CO;
#define REFUSE_FC(h, who)                                                                    \
    CallScope opts_((h)->pending, (h)->call, 0, OPT_FC);                                     \
    if (opts_.refused) return fail(h, GITCAP_ERR_ARG, refused_message(who))

// Pipelined submission: the image pass on the encoder stream, `text_loop` on the slot's decode stream (see gitcap_greedy_submit).
// A failure after the first enqueue must not leave the slot unordered (the next user of the slot waits on ev_dec only): from
// the moment anything may be on the slot's streams, every exit records ev_dec behind BOTH streams' work and marks the slot
// used, and every exit restores slot 0 and the `pipelined` flag.
template <typename TextLoop>
static int submit_common(gitcap* h, FrameSrc src, int B, int F, float* visual_out, hipStream_t stream, int* ticket, TextLoop text_loop) {
    const int slot = ticket_slot(h->next_ticket, gitcap::NSLOT);
    gitcap::Slot& sl = h->slots[slot];
    select_slot(h, slot);
    bool enqueued = false;
    auto leave = [&](int rc) {
        h->pipelined = false;
        if (rc && enqueued) {
            // order the slot behind whatever was enqueued: s_txt waits for the encoder stream, ev_dec is recorded behind both
            if (hipEventRecord(sl.ev_enc, h->s_enc) == hipSuccess) (void)hipStreamWaitEvent(sl.s_txt, sl.ev_enc, 0);
            if (hipEventRecord(sl.ev_dec, sl.s_txt) == hipSuccess) sl.used = true;
            else (void)hipDeviceSynchronize();          // no event to order on: drain instead
            sl.have = false;
        }
        select_slot(h, 0);
        return rc;
    };
#define SUBMIT_OK(expr)                                                                                                \
    do {                                                                                                               \
        hipError_t e_ = (expr);                                                                                        \
        if (e_ != hipSuccess) return leave(fail(h, GITCAP_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_))); \
    } while (0)
    // the image pass may start once the caller's stream has produced `frames` ...
    SUBMIT_OK(hipEventRecord(sl.ev_in, stream));
    SUBMIT_OK(hipStreamWaitEvent(h->s_enc, sl.ev_in, 0));
    // ... and once the previous user of this slot's image K/V (four submissions ago) has finished decoding
    if (sl.used) SUBMIT_OK(hipStreamWaitEvent(h->s_enc, sl.ev_dec, 0));
    h->pipelined = true;
    enqueued = true;
    int rc = encode_impl(h, src, B, F, visual_out, h->s_enc);
    if (rc) return leave(rc);
    SUBMIT_OK(hipEventRecord(sl.ev_enc, h->s_enc));
    SUBMIT_OK(hipStreamWaitEvent(sl.s_txt, sl.ev_enc, 0));
    if ((rc = text_loop(sl.s_txt))) return leave(rc);
    SUBMIT_OK(hipEventRecord(sl.ev_dec, sl.s_txt));
#undef SUBMIT_OK
    sl.used = true;
    *ticket = h->next_ticket++;
    return leave(0);
}


extern "C" {

int gitcap_abi_version(void) { return GITCAP_ABI_VERSION; }

const char* gitcap_last_error(const gitcap_t* h) { return h ? h->err.c_str() : create_err<gitcap>().c_str(); }

int gitcap_create(const gitcap_config* cfg, int device, gitcap_t** out) {
    if (!cfg || !out) return fail<gitcap>(nullptr, GITCAP_ERR_ARG, "create: null argument");
    *out = nullptr;
    const gitcap_config& c = *cfg;
    if (c.patch_size <= 0 || c.image_size % c.patch_size) return fail<gitcap>(nullptr, GITCAP_ERR_ARG, "create: image_size % patch_size != 0");
    if (c.enc_heads * 64 != c.enc_width || c.dec_heads * 64 != c.dec_width)
        return fail<gitcap>(nullptr, GITCAP_ERR_ARG, "create: head_dim must be 64");
    for (int n : {c.enc_width, c.enc_ffn, c.dec_width, c.dec_ffn})
        if (n % 128) return fail<gitcap>(nullptr, GITCAP_ERR_ARG, "create: widths must be multiples of 128");
    if (c.enc_width > 1024) return fail<gitcap>(nullptr, GITCAP_ERR_ARG, "create: enc_width > 1024 unsupported");
    if (!txt_block_ok(c.dec_width)) return fail<gitcap>(nullptr, GITCAP_ERR_ARG, "create: dec_width must be 768 (GIT) or 128 (test config)");
    if (c.max_batch <= 0 || c.max_frames <= 0 || c.max_text_len <= 0 || c.max_beams <= 0)
        return fail<gitcap>(nullptr, GITCAP_ERR_ARG, "create: max_* must be positive");
    if (c.patch_size % 2) return fail<gitcap>(nullptr, GITCAP_ERR_ARG, "create: odd patch_size unsupported");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
        return fail<gitcap>(nullptr, GITCAP_ERR_HIP, "create: no HIP device visible (libgitcap has no CPU path)");
    if (device < 0 || device >= ndev) return fail<gitcap>(nullptr, GITCAP_ERR_ARG, "create: bad device index");
    hipError_t e = hipSetDevice(device);
    if (e != hipSuccess) return fail<gitcap>(nullptr, GITCAP_ERR_HIP, std::string("hipSetDevice: ") + hipGetErrorString(e));

    gitcap* h = new (std::nothrow) gitcap();
    if (!h) return fail<gitcap>(nullptr, GITCAP_ERR_NOMEM, "create: out of host memory");
    h->c = c; h->device = device;
    h->G = c.image_size / c.patch_size; h->N = h->G * h->G + 1;
    h->Kp = pad_to(3 * c.patch_size * c.patch_size, 64);
    h->Dv = c.enc_width; h->D = c.dec_width; h->V = c.vocab_size; h->Vp = pad_to(c.vocab_size, 16);
    h->Smax = c.max_frames * h->N;
    // (+ 256 rows of slack: once needed by the retired 224-row tiles; kept so that the buffer sizes of round 5 stay what they were)
    h->Mi = pad_to(c.max_batch * h->Smax, 256) + 256;
    h->Pp = pad_to(c.max_batch * c.max_frames * h->G * h->G, 256) + 256;
    h->R = c.max_batch * c.max_beams; h->Tmax = c.max_text_len;
    h->Mt = pad_to(h->R * h->Tmax, 16);
    const int Dm = std::max(h->Dv, h->D), Fm = std::max(c.enc_ffn, c.dec_ffn);
    h->nslab_max = std::max(16, std::min(64, c.dec_ffn / 64));    // FC2 partial slabs per text row: dec_ffn / 64 hidden slices (ffn_txt.hip)
    int rc = 0;
    const size_t Mi = h->Mi;
    rc = rc ? rc : dev_alloc(h, &h->x, Mi * Dm);
    rc = rc ? rc : dev_alloc(h, &h->tmp, Mi * h->D);
    rc = rc ? rc : dev_alloc(h, &h->ln_stats, Mi * 16);
    h->ln_cnt_words = 2 * (Mi / 224 + 2);
    rc = rc ? rc : dev_alloc(h, &h->ln_cnt, h->ln_cnt_words);
    if (!rc) {
        if (hipHostMalloc((void**)&h->ln_fail, 64, hipHostMallocMapped) != hipSuccess) rc = fail(h, GITCAP_ERR_NOMEM, "create: hipHostMalloc (exchange flag)");
        else memset(h->ln_fail, 0, 64);
    }
    h->cus = device_cus();
    rc = rc ? rc : dev_alloc(h, &h->hb, Mi * Dm);
    rc = rc ? rc : dev_alloc(h, &h->qkv, Mi * 3 * h->Dv);
    rc = rc ? rc : dev_alloc(h, &h->ctx, Mi * Dm);
    rc = rc ? rc : dev_alloc(h, &h->ffn, Mi * Fm);
    rc = rc ? rc : dev_alloc(h, &h->patches, (size_t)h->Pp * h->Kp);
    for (int i = 0; i < gitcap::NSLOT && !rc; ++i) {
        gitcap::Slot& sl = h->slots[i];
        rc = rc ? rc : dev_alloc(h, &sl.kv_img, (size_t)c.dec_layers * Mi * 3 * h->D);
        rc = rc ? rc : dev_alloc(h, &sl.sep_cnt, (size_t)h->Tmax + 1);
        rc = rc ? rc : dev_alloc(h, &sl.off, (size_t)c.max_batch);
        rc = rc ? rc : dev_alloc(h, &sl.len, (size_t)c.max_batch);
        rc = rc ? rc : dev_alloc(h, &sl.fpos, (size_t)c.max_batch * c.max_frames);
        // Text-row workspace (48 fp32 FC2 slabs + 12 per-head partials = 184 KB per row, the arg-max partials, ...): slot 0 also
        // serves the synchronous entry points, whose teacher-forced passes run rows x positions text rows at once; slots 1-3 only
        // ever run token loops of pipelined submissions -- one position per row and step -- and are sized for that.
        const size_t Mt = i == 0 ? (size_t)h->Mt : (size_t)pad_to(h->R, 16);
        sl.Mt = (int)Mt;
        rc = rc ? rc : dev_alloc(h, &sl.xs, Mt * h->D);
        rc = rc ? rc : dev_alloc(h, &sl.xs2, 2 * h->D);            // second copy of the residual rows for the one/two-row form
        rc = rc ? rc : dev_alloc(h, &sl.slabs, (size_t)h->nslab_max * Mt * h->D);
        rc = rc ? rc : dev_alloc(h, &sl.xsb, Mt * h->D);
        rc = rc ? rc : dev_alloc(h, &sl.part, Mt * (size_t)c.dec_heads * h->D);
        rc = rc ? rc : dev_alloc(h, &sl.row_cnt, Mt);
        rc = rc ? rc : dev_alloc(h, &sl.fs, Mt * c.dec_ffn);
        rc = rc ? rc : dev_alloc(h, &sl.amax_val, Mt * (size_t)((h->V + 15) / 16));
        rc = rc ? rc : dev_alloc(h, &sl.amax_idx, Mt * (size_t)((h->V + 15) / 16));
        rc = rc ? rc : dev_alloc(h, &sl.kv_txt, (size_t)c.dec_layers * h->R * h->Tmax * 3 * h->D);
        rc = rc ? rc : dev_alloc(h, &sl.kv_txt2, (size_t)c.dec_layers * h->R * h->Tmax * 3 * h->D);
        {   // beam-search state: per slot, so that searches of different submissions may be in flight together
            const size_t R = h->R, T = (size_t)h->Tmax + 1, Bm = c.max_batch;
            rc = rc ? rc : dev_alloc(h, &sl.beam.ids0, R * T);
            rc = rc ? rc : dev_alloc(h, &sl.beam.ids1, R * T);
            rc = rc ? rc : dev_alloc(h, &sl.beam.words, R);
            rc = rc ? rc : dev_alloc(h, &sl.beam.hyp_ids, Bm * T);
            rc = rc ? rc : dev_alloc(h, &sl.beam.beam_scores, R);
            rc = rc ? rc : dev_alloc(h, &sl.beam.hyp_score, Bm);
            rc = rc ? rc : dev_alloc(h, &sl.beam.src_rows, R);
            rc = rc ? rc : dev_alloc(h, &sl.beam.done, Bm);
            rc = rc ? rc : dev_alloc(h, &sl.beam.hyp_len, Bm);
            rc = rc ? rc : dev_alloc(h, &sl.beam_logits, R * (size_t)h->V);
            rc = rc ? rc : dev_alloc(h, &sl.cand_scores, Bm * 16);
            rc = rc ? rc : dev_alloc(h, &sl.cand_idx, Bm * 16);
            rc = rc ? rc : dev_alloc(h, &sl.topk_scratch, beam_topk_scratch_bytes(c.max_batch, std::max(1, c.max_beams), h->V, 16));
        }
    }
    if (!rc) {
        // plain non-blocking streams for the pipeline (stream priorities measured neutral and
        // CU-masked streams 2.5x slower on this platform: docs/LAB_NOTEBOOK.md "What did not work")
        bool ok = hipStreamCreateWithFlags(&h->s_enc, hipStreamNonBlocking) == hipSuccess;
        h->n_txt = g_txt_streams;
        for (int i = 0; i < h->n_txt; ++i) ok = ok && hipStreamCreateWithFlags(&h->txt_streams[i], hipStreamNonBlocking) == hipSuccess;
        for (int i = 0; i < gitcap::NSLOT; ++i) h->slots[i].s_txt = h->txt_streams[i % h->n_txt];
        for (auto& sl : h->slots)
            ok = ok && hipEventCreateWithFlags(&sl.ev_in, hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&sl.ev_enc, hipEventDisableTiming) == hipSuccess &&
                 hipEventCreateWithFlags(&sl.ev_dec, hipEventDisableTiming) == hipSuccess;
        if (!ok) rc = fail(h, GITCAP_ERR_HIP, "create: stream/event creation failed");
    }
    if (rc) {
        create_err<gitcap>() = h->err;
        gitcap_destroy(h);
        return rc;
    }
    std::vector<std::pair<std::string, std::vector<int64_t>>> exp;
    expected_shapes(c, exp);
    for (auto& kv : exp) {
        DevTensor t;
        t.shape = kv.second;
        t.kind = is_gemm_weight(kv.first) ? 1 : 0;
        h->w[kv.first] = t;
    }
    *out = h;
    return 0;
}

void gitcap_destroy(gitcap_t* h) {
    if (!h) return;
    for (auto& pc : h->prof)
        for (auto& r : pc.recs) { (void)hipEventDestroy(r.a); (void)hipEventDestroy(r.b); }
    for (auto& sl : h->slots) {
        if (sl.ev_in) (void)hipEventDestroy(sl.ev_in);
        if (sl.ev_enc) (void)hipEventDestroy(sl.ev_enc);
        if (sl.ev_dec) (void)hipEventDestroy(sl.ev_dec);
    }
    for (auto& t : h->txt_streams)
        if (t) (void)hipStreamDestroy(t);
    if (h->s_enc) (void)hipStreamDestroy(h->s_enc);
    h->win_order.destroy();
    if (h->win_ring) (void)hipFree(h->win_ring);
    pool_free(h);
    h->pool_order.destroy();
    free_allocs(*h);
    if (h->ln_fail) (void)hipHostFree(h->ln_fail);
    if (h->acc_host) (void)hipHostFree(h->acc_host);
    if (h->acc_ev) (void)hipEventDestroy(h->acc_ev);
    for (auto& kv : h->w)
        if (kv.second.p) (void)hipFree(kv.second.p);
    for (auto& kv : h->wscale)
        if (kv.second) (void)hipFree(kv.second);
    for (auto& kv : h->wpack)
        if (kv.second.first) (void)hipFree(kv.second.first);
    delete h;
}

int gitcap_load_tensor(gitcap_t* h, const char* name, const float* data, const int64_t* shape, int rank) {
    if (!h || !name || !data || !shape) return fail(h, GITCAP_ERR_ARG, "load_tensor: null argument");
    std::string why;
    DevTensor* tp = find_tensor(h->w, name, shape, rank, "load_tensor", why);
    if (!tp) return fail(h, GITCAP_ERR_ARG, why);
    GUARD(h);
    DevTensor& t = *tp;
    const int64_t rows = rank == 2 ? shape[0] : 1, cols = rank == 2 ? shape[1] : shape[0];
    if (t.p) { (void)hipFree(t.p); t.p = nullptr; h->weight_bytes -= t.bytes; t.bytes = 0; }
    if (t.kind == 1 && h->fp8) {
        // e4m3 storage: one power-of-two scale per row (the smallest that maps the row's amax into +-448), values
        // must already BE e4m3 x 2^k (gitcap.weights.quantize_weights_fp8): this is a lossless re-encoding
        const int64_t prow = pad_to((int)rows, 16), pcol = (strcmp(name, "enc.patch_w") == 0) ? h->Kp : cols;
        std::vector<uint8_t> q((size_t)prow * pcol, 0);
        std::vector<float> sc((size_t)prow, 1.0f);
        for (int64_t r = 0; r < rows; ++r) {
            sc[r] = host_e4m3_row_scale(data + (size_t)r * cols, cols);
            if (!host_e4m3_encode_row(data + (size_t)r * cols, cols, sc[r], q.data() + (size_t)r * pcol))
                return fail(h, GITCAP_ERR_ARG, std::string("load_tensor: ") + name + " holds a value that is not e4m3 x 2^k "
                            "(quantise first: gitcap.weights.quantize_weights_fp8)");
        }
        // the scale buffer is owned by h->wscale from the moment it exists, the codes by t.p: an error below leaks nothing
        float*& dsc = h->wscale[name];
        if (dsc) { (void)hipFree(dsc); dsc = nullptr; }
        HIP_OK(h, hipMalloc((void**)&dsc, sc.size() * 4));
        HIP_OK(h, hipMemcpy(dsc, sc.data(), sc.size() * 4, hipMemcpyHostToDevice));
        HIP_OK(h, hipMalloc(&t.p, q.size()));
        t.bytes = (int64_t)(q.size() + sc.size() * 4);
        h->weight_bytes += t.bytes;
        HIP_OK(h, hipMemcpy(t.p, q.data(), q.size(), hipMemcpyHostToDevice));
    } else if (t.kind == 1) {
        // GEMM weights: bf16, rows padded to 16 (zero rows), patch-embed K padded to a multiple of 64
        if (int rc = upload_bf16_panel(h, t, data, rows, cols, 16, (strcmp(name, "enc.patch_w") == 0) ? h->Kp : cols)) return rc;
        h->weight_bytes += t.bytes;
    } else {
        const size_t bytes = (size_t)rows * cols * 4;
        HIP_OK(h, hipMalloc(&t.p, bytes));
        t.bytes = (int64_t)bytes;
        h->weight_bytes += t.bytes;
        HIP_OK(h, hipMemcpy(t.p, data, bytes, hipMemcpyHostToDevice));
    }
    t.loaded = true;
    h->finalized = false;
    h->n_staged = 0;
    return 0;
}

int gitcap_finalize_weights(gitcap_t* h) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "finalize: null handle");
    GUARD(h);
    for (auto& kv : h->w)
        if (!kv.second.loaded) return fail(h, GITCAP_ERR_STATE, "finalize: tensor '" + kv.first + "' was never loaded");
    auto F = [&](const std::string& n) { return (const float*)h->w[n].p; };
    auto Wt = [&](const std::string& n) {
        WRef r; r.p = h->w[n].p;
        auto it = h->wscale.find(n);
        r.scale = (h->fp8 && it != h->wscale.end()) ? it->second : nullptr;
        return r;
    };
    if (h->fp8) {
        for (auto& kv : h->w)
            if (kv.second.kind == 1 && !h->wscale.count(kv.first))
                return fail(h, GITCAP_ERR_STATE, "finalize: '" + kv.first + "' was loaded before gitcap_set_weight_storage(e4m3)");
        if (!h->wstage) {          // bf16 staging panel of the big-tile GEMMs: the largest weight matrix
            size_t mx = 0;
            for (auto& kv : h->w)
                if (kv.second.kind == 1 && kv.first != "head.w") {
                    const size_t cols = kv.first == "enc.patch_w" ? (size_t)h->Kp : (size_t)kv.second.shape[1];
                    mx = std::max(mx, (size_t)pad_to((int)kv.second.shape[0], 16) * cols);
                }
            int rc = dev_alloc(h, &h->wstage, mx);
            if (rc) return rc;
            auto pe = [](int64_t r, int64_t k) { return (size_t)pad_to((int)r, 16) * (size_t)k; };
            const gitcap_config& c = h->c;
            const size_t enc_l = pe(3 * c.enc_width, c.enc_width) + pe(c.enc_width, c.enc_width) + 2 * pe(c.enc_ffn, c.enc_width);
            const size_t dec_l = pe(3 * c.dec_width, c.dec_width) + pe(c.dec_width, c.dec_width) + 2 * pe(c.dec_ffn, c.dec_width);
            h->lstage_elems = std::max(enc_l, dec_l);
            if ((rc = dev_alloc(h, &h->lstage, h->lstage_elems))) return rc;
        }
    }
    h->patch_w = Wt("enc.patch_w"); h->cls = F("enc.cls"); h->pos = F("enc.pos");
    h->ln_pre_w = F("enc.ln_pre.w"); h->ln_pre_b = F("enc.ln_pre.b");
    h->ln_post_w = F("enc.ln_post.w"); h->ln_post_b = F("enc.ln_post.b");
    h->temporal = F("temporal");
    h->vproj_w = Wt("vproj.w"); h->vproj_b = F("vproj.b"); h->vproj_lnw = F("vproj.ln.w"); h->vproj_lnb = F("vproj.ln.b");
    h->word = F("txt.word"); h->tpos = F("txt.pos"); h->txt_lnw = F("txt.ln.w"); h->txt_lnb = F("txt.ln.b");
    h->head_w = Wt("head.w"); h->head_b = F("head.b");
    h->enc.resize(h->c.enc_layers);
    for (int i = 0; i < h->c.enc_layers; ++i) {
        const std::string p = "enc.L" + std::to_string(i) + ".";
        EncLayer& L = h->enc[i];
        L.ln1w = F(p + "ln1.w"); L.ln1b = F(p + "ln1.b"); L.ln2w = F(p + "ln2.w"); L.ln2b = F(p + "ln2.b");
        L.qkvw = Wt(p + "qkv.w"); L.qkvb = F(p + "qkv.b"); L.projw = Wt(p + "proj.w"); L.projb = F(p + "proj.b");
        L.fc1w = Wt(p + "fc1.w"); L.fc1b = F(p + "fc1.b"); L.fc2w = Wt(p + "fc2.w"); L.fc2b = F(p + "fc2.b");
    }
    h->dec.resize(h->c.dec_layers);
    for (int i = 0; i < h->c.dec_layers; ++i) {
        const std::string p = "dec.L" + std::to_string(i) + ".";
        DecLayer& L = h->dec[i];
        L.qkvw = Wt(p + "qkv.w"); L.qkvb = F(p + "qkv.b"); L.aow = Wt(p + "ao.w"); L.aob = F(p + "ao.b");
        L.ln1w = F(p + "ln1.w"); L.ln1b = F(p + "ln1.b"); L.fc1w = Wt(p + "fc1.w"); L.fc1b = F(p + "fc1.b");
        L.fc2w = Wt(p + "fc2.w"); L.fc2b = F(p + "fc2.b"); L.ln2w = F(p + "ln2.w"); L.ln2b = F(p + "ln2.b");
    }
    // fragment-major copies of the matrices the token loop streams (decoder layers + vocabulary head): what a lane of the
    // text kernels loads per k-step becomes contiguous, a wave instruction reads 1 KiB in one piece (rowops.hip:
    // pack_frags_kernel; 3-4 x the per-CU pull rate).  The image pass keeps reading the row-major originals.
    for (auto& L : h->dec) L.qkvw.pk = L.aow.pk = L.fc1w.pk = L.fc2w.pk = nullptr;
    h->head_w.pk = nullptr;
    if (g_wpack) {
        auto pack = [&](const std::string& n, WRef& r) -> int {
            const DevTensor& t = h->w[n];
            const int rows16 = pad_to((int)t.shape[0], 16), K = (int)t.shape[1];
            const size_t bytes = (size_t)rows16 * K * (r.scale ? 1 : 2);
            auto& slot = h->wpack[n];
            if (slot.first && slot.second != bytes) { (void)hipFree(slot.first); h->ws_bytes -= (int64_t)slot.second; slot = {nullptr, 0}; }
            if (!slot.first) {
                if (hipMalloc(&slot.first, bytes) != hipSuccess) return fail(h, GITCAP_ERR_NOMEM, "finalize: hipMalloc (packed weights)");
                slot.second = bytes;
                h->ws_bytes += (int64_t)bytes;
            }
            HIP_OK(h, launch_pack_frags(r.p, slot.first, rows16, K, r.scale ? 1 : 2, nullptr));
            r.pk = slot.first;
            return 0;
        };
        int rc = 0;
        for (int i = 0; i < h->c.dec_layers && !rc; ++i) {
            const std::string p = "dec.L" + std::to_string(i) + ".";
            DecLayer& L = h->dec[i];
            rc = pack(p + "qkv.w", L.qkvw);
            rc = rc ? rc : pack(p + "ao.w", L.aow);
            rc = rc ? rc : pack(p + "fc1.w", L.fc1w);
            rc = rc ? rc : pack(p + "fc2.w", L.fc2w);
        }
        rc = rc ? rc : pack("head.w", h->head_w);
        if (rc) return rc;
    }
    h->n_staged = 0;
    HIP_OK(h, hipDeviceSynchronize());
    h->finalized = true;
    return 0;
}

int gitcap_encode(gitcap_t* h, const float* frames, int B, int F, float* visual_out, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "encode: null handle");
    CallScope opts(h->pending, h->call, OPT_FC, 0);
    GUARD(h);
    POLL(h);
    return encode_sync(h, FrameSrc{frames, nullptr, 0, 0}, B, F, visual_out, (hipStream_t)stream);
}

// The encoder half of the image pass: B x F frames (checked by the caller) through patch gather, the ViT blocks and ln_post.
// Its output: the bf16 rows in h->hb (the decoder input) and, when ln_f32 != nullptr, the fp32 rows [B*F*N][Dv] there; addv
// (nullable) = the temporal embedding, added to both inside the ln_post epilogue (frame = (row / N) % F).  Touches the encoder
// workspace only (not the image K/V, the text rows or the slot's `have`).  taps: gitcap_dbg_enc_tap may copy the residual stream.
static int encode_frames(gitcap* h, FrameSrc src, int B, int F, float* ln_f32, const float* addv, bool taps, hipStream_t stream) {
    int rc;
    hipStream_t s = stream;
    const gitcap_config& c = h->c;
    const int Dv = h->Dv, N = h->N, nf = B * F, rows = nf * N, Mp = pad_to(rows, 256);
    const int P = nf * h->G * h->G, Pp = pad_to(P, 256);
    h->n_staged = 0;             // nothing staged yet in this pass (a stale entry could match a recycled address)

    // patchify (conv k = stride = p, no bias) + CLS + position embedding, then ln_pre
    if (src.u8) {     // raw camera frames: resize + crop + BGR->RGB + normalise fused with the patch gather (no fp32 frames)
        hipError_t e = launch_preprocess_patches(src.u8, h->patches, nf, src.H, src.W, c.image_size, c.patch_size, h->Kp, s);
        if (e == hipErrorInvalidValue) return fail(h, GITCAP_ERR_ARG, "encode_raw: frames smaller than the crop, or bad sizes");
        HIP_OK(h, e);
    } else {
        HIP_OK(h, launch_im2col(src.f32, h->patches, nf, c.image_size, c.patch_size, h->Kp, s));
    }
    {
        GemmArgs a{};
        HIP_OK(h, resolve_weight(h, h->patch_w, Dv, h->Kp, s, &a.W));
        ProfScope ps(h, GITCAP_PROF_GEMM, s, 2.0 * P * Dv * (3.0 * c.patch_size * c.patch_size), 2.0 * P * h->Kp + 2.0 * Dv * h->Kp + 4.0 * P * Dv);
        a.A = h->patches; a.lda = h->Kp; a.bias = nullptr; a.M = Pp; a.N = Dv; a.K = h->Kp;
        a.out = h->x; a.ldo = Dv; a.pos = h->pos; a.tokens_per_frame = N; a.patches_per_frame = h->G * h->G; a.valid_rows = P;
        HIP_OK(h, launch_gemm_auto(h, a, EPI_PATCH_F32, s));
    }
    // ln_pre (fp32, in place: the residual stream) and the first block's LN1 (bf16: the first q|k|v operand) in one pass;
    // the same pass supplies the CLS rows (cls + pos[0], row frame * N) that the patch GEMM does not write
    {
        const bool canon = Dv == 64 || Dv == 128 || Dv == 256 || Dv == 512 || Dv == 768 || Dv == 1024;
        if (canon) {
            ProfScope ps(h, GITCAP_PROF_ROWOPS, s, 0.0, (double)rows * Dv * 10.0);
            LnArgs a{h->x, Dv, h->ln_pre_w, h->ln_pre_b, c.enc_ln_eps, rows, Dv, h->x, Dv, h->hb, Dv, nullptr, 1, 1,
                     h->enc[0].ln1w, h->enc[0].ln1b, c.enc_ln_eps, h->cls, h->pos, N};
            HIP_OK(h, launch_layernorm(a, s));
        } else {
            {
                ProfScope ps(h, GITCAP_PROF_ROWOPS, s, 0.0, (double)rows * Dv * 8.0);
                LnArgs a{h->x, Dv, h->ln_pre_w, h->ln_pre_b, c.enc_ln_eps, rows, Dv, h->x, Dv, nullptr, 0, nullptr, 1, 1,
                         nullptr, nullptr, 0.f, h->cls, h->pos, N};
                HIP_OK(h, launch_layernorm(a, s));
            }
            if ((rc = ln(h, s, h->x, Dv, h->enc[0].ln1w, h->enc[0].ln1b, c.enc_ln_eps, rows, Dv, nullptr, 0, h->hb, Dv))) return rc;
        }
    }

    // gitcap_dbg_enc_tap (synchronous calls only): the residual stream entering block e
    auto tap = [&](int e) -> hipError_t {
        return (taps && h->enc_tap && h->cur_slot == 0 && !h->pipelined && e < c.enc_layers)
                   ? hipMemcpyAsync(h->enc_tap + (size_t)e * rows * Dv, h->x, (size_t)rows * Dv * 4, hipMemcpyDeviceToDevice, s) : hipSuccess;
    };
    HIP_OK(h, tap(0));
    // pre-LN blocks: x += proj(attn(LN1 x)); x += fc2(qgelu(fc1(LN2 x))).  Each residual GEMM also produces the
    // LayerNorm its consumer needs (LN2 of this block / LN1 of the next; the last one ln_post + temporal embedding); the first
    // LN1 came out of the ln_pre pass above.
    const bool f8 = use_f8(h);
    for (int i = 0; i < c.enc_layers; ++i) {
        const EncLayer& L = h->enc[i];
        {   // e4m3 storage: the layer's matrices -> bf16 staging, one launch (fp8 compute reads FC1 / FC2 as they are)
            const WRef* ws[4] = {&L.qkvw, &L.projw, &L.fc1w, &L.fc2w};
            const int wr[4] = {3 * Dv, Dv, c.enc_ffn, Dv}, wk[4] = {Dv, Dv, Dv, c.enc_ffn};
            if ((rc = stage_layer(h, s, ws, wr, wk, f8 ? 2 : 4))) return rc;
        }
        if ((rc = gemm(h, s, EPI_BIAS_BF16, h->hb, Dv, L.qkvw, L.qkvb, rows, Mp, 3 * Dv, Dv, h->qkv, 3 * Dv))) return rc;
        {
            ProfScope ps(h, GITCAP_PROF_ATTN_FULL, s, 4.0 * nf * c.enc_heads * (double)N * N * 64, 0.0);
            HIP_OK(h, launch_attn_full(h->qkv, h->ctx, nf, N, c.enc_heads, s));
        }
        LnOpts proj; proj.ln8 = f8 ? h->hb8 : nullptr;
        if ((rc = gemm_ln(h, s, false, h->ctx, Dv, L.projw, L.projb, Mp, Dv, Dv, h->x, h->x, L.ln2w, L.ln2b, c.enc_ln_eps, rows,
                          h->hb, nullptr, proj))) return rc;
        // FC1 + QuickGELU, FC2 (+ the next LayerNorm): bf16, or (compute = fp8_ffn) on e4m3 operands at twice the MFMA rate
        const bf16_t* fc2_in = f8 ? (const bf16_t*)h->ffn8 : h->ffn;
        if (f8) rc = gemm_f8(h, s, EPI_BIAS_QGELU_F8, h->hb8, Dv, L.fc1w, L.fc1b, rows, Mp, c.enc_ffn, Dv, h->ffn8, c.enc_ffn);
        else rc = gemm(h, s, EPI_BIAS_QGELU_BF16, h->hb, Dv, L.fc1w, L.fc1b, rows, Mp, c.enc_ffn, Dv, h->ffn, c.enc_ffn);
        if (rc) return rc;
        LnOpts fc2; fc2.f8in = f8;
        if (i + 1 < c.enc_layers) {
            const EncLayer& Nx = h->enc[i + 1];
            if ((rc = gemm_ln(h, s, false, fc2_in, c.enc_ffn, L.fc2w, L.fc2b, Mp, Dv, c.enc_ffn, h->x, h->x, Nx.ln1w, Nx.ln1b,
                              c.enc_ln_eps, rows, h->hb, nullptr, fc2))) return rc;
            HIP_OK(h, tap(i + 1));
        } else {
            // the last block's FC2 is followed by ln_post (+ per-frame temporal embedding, model.py:380); frames of a clip are
            // already adjacent rows, so the concat along tokens (model.py:382) is the identity on this layout.  x itself is
            // not needed any more.  The fp32 visual features (58 MB at B=16, F=6) are written straight into the caller's
            // buffer and only when asked for; the decoder consumes the bf16 copy.
            fc2.addv = addv; fc2.add_div = N; fc2.add_mod = F; fc2.ln_f32 = ln_f32;
            if ((rc = gemm_ln(h, s, false, fc2_in, c.enc_ffn, L.fc2w, L.fc2b, Mp, Dv, c.enc_ffn, nullptr, h->x, h->ln_post_w, h->ln_post_b,
                              c.enc_ln_eps, rows, h->hb, nullptr, fc2))) return rc;
        }
    }
    return 0;
}

static int encode_impl(gitcap* h, FrameSrc src, int B, int F, float* visual_out, hipStream_t stream) {
    int rc = src.u8 ? check_frames(h, src.u8, B, F, true) : check_frames(h, src.f32, B, F);
    if (rc) return rc;
    cur(h).have = false;
    if (const RaggedCounts& fc = h->call.fc; fc.B != 0) {
        // packed clips: `frames` holds sum(counts) frames, F is the largest count
        if (fc.B != B) return fail(h, GITCAP_ERR_ARG, "encode: B differs from the attached frame counts'");
        int total = 0, mx = 0, mn = 256;
        for (int b = 0; b < B; ++b) { total += fc.n[b]; mx = std::max(mx, (int)fc.n[b]); mn = std::min(mn, (int)fc.n[b]); }
        if (mx != F) return fail(h, GITCAP_ERR_ARG, "encode: F is not the largest of the attached frame counts");
        if (total > h->c.max_batch * h->c.max_frames) return fail(h, GITCAP_ERR_ARG, "encode: the attached frame counts sum beyond max_batch * max_frames");
        if (mn != mx) {
            gitcap::Slot& sl = cur(h);
            const int N = h->N;
            HIP_OK(h, launch_ragged_tables(fc, N, sl.off, sl.len, sl.fpos, stream));
            if (h->c.num_frames > 0) {
                // every frame is encoded on its own without the fused temporal add; the fp32 ln_post rows are staged in the q|k|v
                // buffer (dead behind the last block's attention, as in window_push) and the row kernel adds temporal[pos[frame]]
                float* stage = (float*)h->qkv;
                if ((rc = encode_frames(h, src, total, 1, stage, nullptr, true, stream))) return rc;
                const double rows = (double)total * N;
                ProfScope ps(h, GITCAP_PROF_ROWOPS, stream, 0.0, rows * h->Dv * (4.0 + 2.0 + (visual_out ? 4.0 : 0.0)));
                HIP_OK(h, launch_ragged_temporal(stage, h->temporal, sl.fpos, h->hb, visual_out, total, N, h->Dv, stream));
            } else if ((rc = encode_frames(h, src, total, 1, visual_out, nullptr, true, stream))) return rc;
            return image_prefix(h, B, F * N, stream, total * N);
        }
        // equal counts: the dense path, launch for launch
    }
    if ((rc = encode_frames(h, src, B, F, visual_out, h->c.num_frames > 0 ? h->temporal : nullptr, true, stream))) return rc;
    return image_prefix(h, B, F * h->N, stream);
}

// a synchronous call's image pass: slot 0, the caller's stream, behind the submissions in flight
static int encode_sync(gitcap* h, FrameSrc src, int B, int F, float* visual_out, hipStream_t s) {
    select_slot(h, 0);
    HIP_OK(h, join_async(h, s));
    return encode_impl(h, src, B, F, visual_out, s);
}

int gitcap_set_visual(gitcap_t* h, const float* visual, int B, int S_img, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "set_visual: null handle");
    REFUSE_FC(h, "set_visual");
    GUARD(h);
    POLL(h);
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "weights not finalized");
    select_slot(h, 0);
    if (!visual || B <= 0 || S_img <= 0) return fail(h, GITCAP_ERR_ARG, "set_visual: bad arguments");
    if (B > h->c.max_batch || S_img > h->Smax) return fail(h, GITCAP_ERR_ARG, "set_visual: B/S_img exceed the sizes the handle was created for");
    if (((uintptr_t)visual & 15) != 0) return fail(h, GITCAP_ERR_ARG, "set_visual: visual must be 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    cur(h).have = false;
    HIP_OK(h, join_async(h, s));
    HIP_OK(h, launch_cast_bf16(visual, h->hb, (int64_t)B * S_img * h->Dv, s));
    return image_prefix(h, B, S_img, s);
}

int gitcap_text_forward(gitcap_t* h, const int64_t* ids, int ld_ids, int rows, int beams, int t0, int T,
                        float* logits_out, int all_positions, int64_t* argmax_out, int ld_argmax, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "text_forward: null handle");
    GUARD(h);
    POLL(h);
    select_slot(h, 0);
    HIP_OK(h, join_async(h, (hipStream_t)stream));
    TextReq q;
    q.ids = ids; q.ld_ids = ld_ids; q.rows = rows; q.beams = beams; q.t0 = t0; q.T = T;
    q.logits_out = logits_out; q.all_positions = all_positions; q.argmax_out = argmax_out; q.ld_argmax = ld_argmax;
    return text_forward(h, q, (hipStream_t)stream);
}

// token steps t_first .. max_len-1 of `rows` text rows (the image K/V of their clips in the selected slot), ids at ids_out (row pitch ld)
// The call's options (h->call): lp (row pitch lp.ld): column t = the log-probability of the token step t emitted; pr: steps that
// write a position inside a row's prompt take the prompt's token there (launch_argmax_final); co: the constraints
// tail (nullable; a verified draft's, host_logic.h): the steps that write a position some row holds already run the KEEP arg-max
// against the slot's keep_len
static int greedy_rows(gitcap* h, int rows, int max_len, int64_t* ids_out, int ld, hipStream_t s, int t_first = 0,
                       const DraftTail* tail = nullptr) {
    const LpAttach& lp = h->call.lp;
    const TopkAttach& tk = h->call.tk;                       // column t = the k best of the distribution step t chose from
    const PromptArgs* prompt = h->call.pr.ids ? &h->call.pr : nullptr;
    const bool chain = text_chain_ok(h, rows, 1);
    // (Round 6 folded the arg-max of step t into the q|k|v launch of step t + 1 for one / two rows -- one launch less per step, same
    // bits -- and measured nothing: 4.926 vs 4.912 ms per 20-token caption; tools/experiments/argmax_fold_rows.txt.)
    bool have_rows = false;                                  // the previous step's arg-max launch embedded this step's input rows
    // constraints attached: one small launch per step builds the rows' ban mask from the ids so far (prefix 0 .. t, CLS and prompt
    // included), and the head runs in its BAN form; a position a prompt forces takes the prompt's token whatever is banned
    const ConsOpt& co = h->call.co;
    const HeadBan bn{cur(h).ban_mask, h->ban_ld};
    TextReq q;                                               // what every step shares; the position's part is filled per step
    q.ld_ids = ld; q.rows = rows; q.T = 1; q.ld_argmax = ld; q.sep_cnt = cur(h).sep_cnt; q.ld_lp = lp.ld;
    q.prompt = prompt; q.ban = co.on ? &bn : nullptr;
    for (int t = t_first; t < max_len; ++t) {
        // forward on the sequence so far, argmax of the last position, append (model.py:173-182)
        const bool next = chain && t + 1 < max_len && t + 1 < h->c.max_text_pos;
        if (co.on)
            HIP_OK(h, launch_ban_mask(ids_out, ld, rows, t + 1, co.ngram, co.min_length, h->c.sep_token_id, co.suppress, co.n_suppress,
                                      h->c.vocab_size, cur(h).ban_mask, bn.ld, s));
        q.ids = ids_out + t; q.t0 = q.step = t; q.argmax_out = ids_out + t + 1; q.lp_out = lp.p ? lp.p + t : nullptr;
        if (tk.k) q.topk = TopkAttach{tk.k, tk.ids + (size_t)t * tk.k, tk.lp + (size_t)t * tk.k, tk.ld};
        q.pre_embedded = have_rows; q.embed_next = next;
        q.keep_len = tail && draft_keep_step(*tail, t) ? cur(h).keep_len : nullptr;
        if (const int rc = text_forward(h, q, s)) return rc;
        have_rows = next;
    }
    return 0;
}

// (Round 4 ran a synchronous call's loop as two / three / four part-batch loops side by side on the decode streams --
// clips are independent, every kernel is batch invariant, the captions were bitwise the same: 16 clips 323-325 / 580 / 600 us
// per token step against 302 for one loop (profiles/r04_sync_call_split_token_loop.txt).  Chains of ~6 us launches on
// different streams do not overlap each other the way one chain overlaps an image pass.  Removed.)
static int greedy_text_loop(gitcap* h, int B, int max_len, int stop, int64_t* ids_out, int32_t* steps_out, hipStream_t s) {
    const LpAttach& lp = h->call.lp;
    const PromptArgs& pr = h->call.pr;
    const int ld = max_len + 1;
    gitcap::Slot& sl = cur(h);
    int rc;
    HIP_OK(h, hipMemsetAsync(sl.sep_cnt, 0, ((size_t)h->Tmax + 1) * 4, s));
    if (!pr.ids) {
        // CLS start tokens [B,1] (model.py:171)
        HIP_OK(h, launch_fill_i64(ids_out, ld, B, h->c.cls_token_id, s));
        if ((rc = greedy_rows(h, B, max_len, ids_out, ld, s))) return rc;
    } else {
        // the prompts [B, lengths[b]] in place of the lone CLS (model.py:432-437)
        HIP_OK(h, launch_fill_prompt(ids_out, ld, B, pr, s));
        // positions 0 .. min_len-1 are prompt in every row: one multi-position pass (its arg-max is step min_len-1's), where the
        // slot's row workspace holds B x min_len rows; the token loop goes on behind it.  Steps that write a position below the
        // longest prompt run the forced arg-max.
        // (with constraints attached the prompt runs as forced steps: the one-pass plan is not combined with the ban mask; with top-k
        // alternatives attached too: every forced position reports the model's own ranks, which needs that position's head)
        const int P = (g_prompt_prefill && !h->call.co.on && !h->call.tk.k && pr.min_len > 1 && (int64_t)B * pr.min_len <= sl.Mt) ? std::min(pr.min_len, max_len) : 1;
        int t_first = 0;
        if (P > 1) {
            if (lp.p) HIP_OK(h, hipMemset2DAsync(lp.p, (size_t)lp.ld * 4, 0, (size_t)(P - 1) * 4, B, s));    // forced positions: 0.0f
            TextReq q;
            q.ids = ids_out; q.ld_ids = ld; q.rows = B; q.T = P;
            q.argmax_out = ids_out + P; q.ld_argmax = ld; q.sep_cnt = sl.sep_cnt; q.step = P - 1;
            q.lp_out = lp.p ? lp.p + (P - 1) : nullptr; q.ld_lp = lp.ld; q.prompt = &pr;
            if ((rc = text_forward(h, q, s))) return rc;
            t_first = P;
        }
        if ((rc = greedy_rows(h, B, max_len, ids_out, ld, s, t_first))) return rc;
    }
    if (steps_out) HIP_OK(h, launch_finish_steps(sl.sep_cnt, B, max_len, stop, steps_out, s));
    return 0;
}

// ---- greedy decoding that verifies a draft caption, accepted row by row ------------------------------------------------------
// A cached token step is bit for bit the teacher-forced position (the prompt plan above relies on it) and a row does not depend on
// the rows beside it.  So the tokens the loop emits after CLS, d_1 .. d_j are the head's arg-max at position j of ONE pass over the
// draft, and every caption keeps its own leading matches (launch_draft_accept_rows; the first position that differs holds the
// loop's own token).  The loop goes on at the first step some caption lacks; captions ahead of it keep their tokens (KEEP arg-max)
// and recompute K/V from them.  The call's options: lp only (a prompt or constraints are refused by the entry points).
static int ensure_draft(gitcap* h) {
    gitcap::Slot& sl = h->slots[0];
    const size_t Bm = (size_t)h->c.max_batch;
    if (!h->acc_host) {
        HIP_OK(h, hipHostMalloc((void**)&h->acc_host, (4 + Bm) * 4, hipHostMallocMapped));
        HIP_OK(h, hipEventCreateWithFlags(&h->acc_ev, hipEventDisableTiming));
    }
    int rc = 0;
    if (!sl.acc_tok) rc = dev_alloc(h, &sl.acc_tok, (size_t)sl.Mt);
    if (!rc && !sl.acc_lp) rc = dev_alloc(h, &sl.acc_lp, (size_t)sl.Mt);
    if (!rc && !sl.acc_row) rc = dev_alloc(h, &sl.acc_row, 2 * Bm);
    if (!rc && !sl.acc_ticket) rc = dev_alloc(h, &sl.acc_ticket, 1 + Bm);
    if (!rc && !sl.keep_len) rc = dev_alloc(h, &sl.keep_len, Bm);
    return rc;
}
static int greedy_draft_loop(gitcap* h, int B, const Draft& d, int max_len, int stop, int64_t* ids_out, int32_t* steps_out, hipStream_t s) {
    const LpAttach& lp = h->call.lp;
    const int ld = max_len + 1, n = d.n;
    gitcap::Slot& sl = cur(h);
    int rc;
    if (n > 63 || (int64_t)B * n > sl.Mt) {      // beyond the accept launch / the slot's row workspace: the plain loop, nothing offered
        if ((rc = greedy_text_loop(h, B, max_len, stop, ids_out, steps_out, s))) return rc;
        if (d.accepted_out) std::fill(d.accepted_out, d.accepted_out + B, 0);
        ++h->draft_calls;
        return 0;
    }
    if ((rc = ensure_draft(h))) return rc;
    // 1. stage; 2. verify: one pass over positions 0 .. n-1 (their K/V rows -> the cache), the head's partials of all B * n rows
    HIP_OK(h, hipMemsetAsync(sl.sep_cnt, 0, ((size_t)h->Tmax + 1) * 4, s));
    HIP_OK(h, launch_draft_stage(d.ids, d.ld, n, B, h->c.vocab_size, h->c.cls_token_id, ids_out, ld, s));
    {
        TextReq q;
        q.ids = ids_out; q.ld_ids = ld; q.rows = B; q.T = n; q.verify = true; q.verify_lp = lp.p != nullptr;
        if ((rc = text_forward(h, q, s))) return rc;
    }
    // 3. accept, and the call's one host wait
    volatile int32_t* host = h->acc_host;
    host[0] = -1;
    DraftAcceptRowsArgs da{};
    da.val = sl.amax_val; da.idx = sl.amax_idx; da.ntiles = (h->V + 15) / 16; da.B = B; da.n = n; da.ids = ids_out; da.ld = ld;
    da.len = sl.keep_len; da.tok = sl.acc_tok; da.row_res = sl.acc_row; da.ticket = sl.acc_ticket; da.sep_cnt = sl.sep_cnt;
    da.sep_id = h->c.sep_token_id; da.host = h->acc_host; da.host_rows = h->acc_host + 4;
    if (lp.p) { da.sum = sl.amax_sum; da.lp_tok = sl.acc_lp; da.lp_out = lp.p; da.ld_lp = lp.ld; }
    HIP_OK(h, launch_draft_accept_rows(da, s));
    HIP_OK(h, hipEventRecord(h->acc_ev, s));
    HIP_OK(h, hipEventSynchronize(h->acc_ev));
    const int cmin = host[0], cmax = host[1], asum = host[2];
    if (cmin < 1 || cmin > cmax || cmax > n) return fail(h, GITCAP_ERR_HIP, "greedy_draft: the accept kernel published no count");
    // 4. tail: the token steps some caption lacks; 5. finish
    const DraftTail tail = draft_tail_plan(cmin, cmax, host[3] != 0, max_len, stop == GITCAP_STOP_ALL_SEP);
    if (tail.run && (rc = greedy_rows(h, B, max_len, ids_out, ld, s, tail.t_first, &tail))) return rc;
    if (steps_out) HIP_OK(h, launch_finish_steps(sl.sep_cnt, B, max_len, stop, steps_out, s));
    if (d.accepted_out)
        for (int r = 0; r < B; ++r) d.accepted_out[r] = host[4 + r];
    ++h->draft_calls; h->draft_offered += (int64_t)n * B; h->draft_accepted += asum; h->draft_tail_steps += tail.steps;
    return 0;
}

}  // extern "C"

// The call's constraints refuse a call whose rows could lose every column: each step bans at most n_suppress listed ids, one id per
// prefix position and SEP.
static int cons_check(gitcap* h, int max_len, int need, const char* who) {
    const ConsOpt& co = h->call.co;
    if (co.on && (int64_t)co.n_suppress + max_len + need > h->c.vocab_size)
        return fail(h, GITCAP_ERR_ARG, std::string(who) + ": the attached constraints could ban every column of a row (n_suppress + max_len >= vocab_size)");
    return 0;
}

// The head of every greedy-family entry point: the null check (its message names the entry point), the pending attachments in
// `take` become the call's options (a call refused below has consumed them), device, exchange health, the argument checks; then
// body().  refuse: the window call's OPT_FC -- it fails where its image prefix would start.
template <typename Body>
static int greedy_entry(gitcap* h, bool args_ok, const char* null_msg, unsigned take, unsigned refuse, int max_len, int stop,
                        const int64_t* ids_out, Body body) {
    if (!h || !args_ok) return fail(h, GITCAP_ERR_ARG, null_msg);
    CallScope opts(h->pending, h->call, take, refuse);
    const LpAttach& lp = h->call.lp;
    const PromptArgs& pr = h->call.pr;
    GUARD(h);
    POLL(h);
    if (!ids_out || max_len <= 0) return fail(h, GITCAP_ERR_ARG, "greedy: bad arguments");
    if (max_len > h->Tmax) return fail(h, GITCAP_ERR_ARG, "greedy: max_len exceeds max_text_len");
    if (stop != GITCAP_STOP_NEVER && stop != GITCAP_STOP_ALL_SEP) return fail(h, GITCAP_ERR_ARG, "greedy: unknown stop rule");
    if (pr.ids && pr.max_len > max_len) return fail(h, GITCAP_ERR_ARG, "greedy: the attached prompt is longer than max_len");
    if (int rc = lp_check(h, "greedy", lp, max_len)) return rc;
    if (int rc = tk_check(h, "greedy", h->call.tk, max_len)) return rc;
    if (int rc = cons_check(h, max_len, 1, "greedy")) return rc;
    if (opts.refused & OPT_FC) return fail(h, GITCAP_ERR_ARG, refused_message("window"));
    if (opts.refused & OPT_TK)      // (the entry point's own name: what null_msg leads with, "greedy_draft" or "window_greedy_draft")
        return fail(h, GITCAP_ERR_ARG, refused_message(std::string(null_msg, strcspn(null_msg, ":")).c_str(), OPT_TK));
    if (opts.refused) return fail(h, GITCAP_ERR_ARG, "greedy_draft: a prompt or constraints are attached, which a draft call does not take");
    return body();
}

// the draft forms: log-probabilities (and, with an image pass of their own, frame counts) are taken, a pending prompt or pending
// constraints are consumed and the call fails; synchronous only (the accept step waits on the host).  prefix(): the image pass.
template <typename Prefix>
static int greedy_draft_entry(gitcap* h, const char* null_msg, unsigned take, unsigned refuse, const Draft& d, int max_len, int stop,
                              int64_t* ids_out, int32_t* steps_out, hipStream_t s, Prefix prefix) {
    return greedy_entry(h, true, null_msg, take, refuse | OPT_PR | OPT_CO | OPT_TK, max_len, stop, ids_out, [&]() -> int {
        if (!d.ids) return fail(h, GITCAP_ERR_ARG, "greedy_draft: null draft_ids");
        if (d.n < 1 || d.n > max_len || d.ld < d.n + 1)
            return fail(h, GITCAP_ERR_ARG, "greedy_draft: n_draft outside [1, max_len], or ld_draft < n_draft + 1");
        if (int rc = prefix()) return rc;
        return greedy_draft_loop(h, cur(h).B, d, max_len, stop, ids_out, steps_out, s);
    });
}

// synchronous: image pass and token loop on the caller's stream, slot 0 (a raw source is checked by the image pass alone)
static int greedy_sync(gitcap* h, const char* null_msg, FrameSrc src, int B, int F, int max_len, int stop, int64_t* ids_out,
                       int32_t* steps_out, hipStream_t s) {
    return greedy_entry(h, true, null_msg, TAKE_GREEDY | OPT_FC, 0, max_len, stop, ids_out, [&]() -> int {
        if (int rc = encode_sync(h, src, B, F, nullptr, s)) return rc;
        return greedy_text_loop(h, B, max_len, stop, ids_out, steps_out, s);
    });
}

// submitted: lp's buffer stays valid until the wait, like ids_out; raw: camera frames, checked before the submission takes a slot
static int greedy_submit(gitcap* h, const char* null_msg, FrameSrc src, bool raw, int B, int F, int max_len, int stop, int64_t* ids_out,
                         int32_t* steps_out, hipStream_t stream, int* ticket) {
    return greedy_entry(h, ticket != nullptr, null_msg, TAKE_GREEDY | OPT_FC, 0, max_len, stop, ids_out, [&]() -> int {
        if (int rc = raw ? check_raw(h, src.u8, B, F, src.H, src.W) : 0) return rc;
        return submit_common(h, src, B, F, nullptr, stream, ticket, [&](hipStream_t s) {
            return greedy_text_loop(h, B, max_len, stop, ids_out, steps_out, s);
        });
    });
}

extern "C" {

int gitcap_greedy(gitcap_t* h, const float* frames, int B, int F, int max_len, int stop, int64_t* ids_out, int32_t* steps_out, void* stream) {
    return greedy_sync(h, "greedy: null handle", FrameSrc{frames, nullptr, 0, 0}, B, F, max_len, stop, ids_out, steps_out, (hipStream_t)stream);
}

int gitcap_encode_raw(gitcap_t* h, const uint8_t* frames_hwc_bgr, int B, int F, int H, int W, float* visual_out, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "encode_raw: null handle");
    CallScope opts(h->pending, h->call, OPT_FC, 0);
    GUARD(h);
    POLL(h);
    return encode_sync(h, FrameSrc{nullptr, frames_hwc_bgr, H, W}, B, F, visual_out, (hipStream_t)stream);
}

int gitcap_greedy_raw(gitcap_t* h, const uint8_t* frames_hwc_bgr, int B, int F, int H, int W, int max_len, int stop,
                      int64_t* ids_out, int32_t* steps_out, void* stream) {
    return greedy_sync(h, "greedy_raw: null handle", FrameSrc{nullptr, frames_hwc_bgr, H, W}, B, F, max_len, stop, ids_out, steps_out, (hipStream_t)stream);
}

int gitcap_greedy_submit(gitcap_t* h, const float* frames, int B, int F, int max_len, int stop, int64_t* ids_out,
                         int32_t* steps_out, void* stream, int* ticket) {
    return greedy_submit(h, "greedy_submit: null argument", FrameSrc{frames, nullptr, 0, 0}, false, B, F, max_len, stop, ids_out, steps_out,
                         (hipStream_t)stream, ticket);
}

int gitcap_greedy_raw_submit(gitcap_t* h, const uint8_t* frames_hwc_bgr, int B, int F, int H, int W, int max_len, int stop,
                             int64_t* ids_out, int32_t* steps_out, void* stream, int* ticket) {
    return greedy_submit(h, "greedy_raw_submit: null argument", FrameSrc{nullptr, frames_hwc_bgr, H, W}, true, B, F, max_len, stop, ids_out,
                         steps_out, (hipStream_t)stream, ticket);
}

int gitcap_greedy_wait(gitcap_t* h, int ticket, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "greedy_wait: null handle");
    GUARD(h);
    POLL(h);
    if (!ticket_waitable(ticket, h->next_ticket, gitcap::NSLOT))
        return fail(h, GITCAP_ERR_ARG, "greedy_wait: ticket is not one of the submissions in flight");
    if (ticket_poisoned(ticket, h->poison_upto))
        return fail(h, GITCAP_ERR_EXCHANGE, "this submission was in flight when a GEMM + LayerNorm launch timed out waiting for its sibling "
                    "tiles: its results are undefined -- submit it again (the handle now uses separate LayerNorm launches)");
    HIP_OK(h, hipStreamWaitEvent((hipStream_t)stream, h->slots[ticket_slot(ticket, gitcap::NSLOT)].ev_dec, 0));
    return 0;
}

// The search loop over the image K/V of the selected slot (its beam state, text K/V and row workspace), on stream s.
// step_logits_out (nullable): [max_steps - 1][B * beams][V], the raw logits of every step (what model.py:521 saves).
// so (h->call.so): the call's search options.  rp != 1: the candidates are ranked on the logits penalised at the columns of every row's prefix
// (the saved step logits stay raw, model.py:521 comes before :522); n > 1: the bookkeeping keeps n hypotheses in the slot's nb_* state.
// decoded_out / logprobs_out receive rank 0, the attached outputs all n ranks.
static int beam_loop(gitcap* h, int B, int beams, int max_steps, float length_penalty, int per_node_beam_size,
                     int64_t* decoded_out, float* logprobs_out, float* step_logits_out, hipStream_t s) {
    const SearchOpt& so = h->call.so;
    const PromptArgs& pr = h->call.pr;
    const ConsOpt& co = h->call.co;
    const PromptArgs* prompt = pr.ids ? &pr : nullptr;
    const int forced_all = prompt ? pr.min_len : 1;          // steps cur_len < forced_all rank nothing: every clip is inside its prompt
    const int rows = B * beams, K = beams * per_node_beam_size, V = h->c.vocab_size, L = max_steps;
    gitcap::Slot& sl = cur(h);
    int rc;
    BeamBuffers bb = sl.beam;
    if (so.n > 1) { bb.hyp_ids = sl.nb_ids; bb.hyp_score = sl.nb_score; bb.hyp_len = sl.nb_len; }
    HIP_OK(h, launch_beam_init(bb, B, beams, so.n, L, h->c.cls_token_id, s));
    // constraints attached: the mask of the B * beams rows, each from the buffer that holds its current prefix
    const HeadBan bn{sl.ban_mask, h->ban_ld};
    const HeadBan* ban = co.on ? &bn : nullptr;
    // the records of a step: what does not change from step to step is filled here
    TextReq q;                  // one position of every beam row: logits only where the step ranks or the caller keeps them
    q.ids = sl.beam.words; q.ld_ids = 1; q.rows = rows; q.beams = beams; q.T = 1;
    CandArgs ca{};
    ca.ld = V; ca.beam_scores = sl.beam.beam_scores; ca.ld_ids = L; ca.rp = so.rp; ca.B = B; ca.beams = beams; ca.V = V;
    ca.out_scores = sl.cand_scores; ca.out_idx = sl.cand_idx; ca.bn = ban;
    BeamStepArgs st{};
    st.n = so.n; st.cand_scores = sl.cand_scores; st.cand_idx = sl.cand_idx; st.B = B; st.beams = beams; st.K = K; st.V = V;
    st.max_len = L; st.eos = h->c.sep_token_id; st.length_penalty = length_penalty; st.sampled = so.smp.on; st.prompt = prompt;
    // while cur_len < max_length (model.py:518): the token at position cur_len-1 is decoded, candidates for
    // position cur_len are ranked, bookkept and the text K/V rows follow their beams -- no host round trip
    for (int cur_len = 1, cur = 0; cur_len < L; ++cur_len, cur ^= 1) {
        const int t = cur_len - 1;
        const bool ranked = cur_len >= forced_all;
        if (t >= forced_all) {                                               // rows continue beam src_rows[r]: all layers, one launch
                                                                             // (t > 0; behind an all-forced step src_rows is the identity)
            HIP_OK(h, launch_gather_txt_rows(sl.kv_txt, sl.kv_txt2, sl.beam.src_rows, rows, t, h->Tmax, 3 * h->D, h->c.dec_layers,
                                             (size_t)h->R * h->Tmax * 3 * h->D, s));
            std::swap(sl.kv_txt, sl.kv_txt2);
        }
        // (an all-forced step needs the K/V append only: no vocabulary head unless the caller keeps the step logits)
        float* lg = step_logits_out ? step_logits_out + (size_t)t * rows * V : (ranked ? sl.beam_logits : nullptr);
        q.t0 = t; q.logits_out = lg;
        if ((rc = text_forward(h, q, s))) return rc;
        ca.logits = lg; ca.prefix_ids = cur ? sl.beam.ids1 : sl.beam.ids0; ca.cur_len = cur_len;
        if (ranked && ban)
            HIP_OK(h, launch_ban_mask(ca.prefix_ids, L, rows, cur_len, co.ngram, co.min_length, h->c.sep_token_id, co.suppress, co.n_suppress, V,
                                      sl.ban_mask, bn.ld, s));
        if (!ranked) {
        } else if (so.smp.on)                                                       // model.py:532-554: K draws instead of the K best
            HIP_OK(h, launch_sample_rows(ca, per_node_beam_size, so.smp, SampleStats{}, s));
        else
            HIP_OK(h, launch_beam_topk(ca, K, sl.topk_scratch, s));
        st.cur_len = cur_len; st.cur = cur;
        HIP_OK(h, launch_beam_step(bb, st, s));
    }
    HIP_OK(h, launch_beam_finish(bb, so.n, B, L, h->c.sep_token_id, BeamFinishOut{so.nbest, so.nbest_lp, decoded_out, logprobs_out}, s));
    if (h->cur_slot == 0) h->att.permuted = true;       // the text cache's rows followed their beams: no caption's positions in a row
    return 0;
}

int gitcap_beam_search_wait(gitcap_t* h, int ticket, void* stream) { return gitcap_greedy_wait(h, ticket, stream); }

}  // extern "C"

// The head of every beam-search entry point (as greedy_entry): the pending attachments in `take` become the call's options (a call
// refused below has consumed them); then `body()`.
template <typename Body>
static int beam_entry(gitcap* h, bool args_ok, const char* null_msg, unsigned take, unsigned refuse, int beams, int max_steps,
                      int per_node_beam_size, const int64_t* decoded_out, const float* logprobs_out, Body body) {
    if (!h || !args_ok) return fail(h, GITCAP_ERR_ARG, null_msg);
    CallScope opts(h->pending, h->call, take, refuse);
    const SearchOpt& so = h->call.so;
    const PromptArgs& pr = h->call.pr;
    GUARD(h);
    POLL(h);
    if (!decoded_out || !logprobs_out || beams < 1 || per_node_beam_size < 1) return fail(h, GITCAP_ERR_ARG, "beam_search: bad arguments");
    if (beams > h->c.max_beams || beams > 16 || beams * per_node_beam_size > 16)
        return fail(h, GITCAP_ERR_ARG, "beam_search: beams exceed max_beams / 16 candidates");
    if (max_steps < 2 || max_steps > h->Tmax) return fail(h, GITCAP_ERR_ARG, "beam_search: max_steps outside [2, max_text_len]");
    if (pr.ids && pr.max_len > max_steps - 1) return fail(h, GITCAP_ERR_ARG, "beam_search: the attached prompt is longer than max_steps - 1");
    // with fewer than 2 candidates per beam one EOS candidate leaves a sentence short of `beams` live beams, which the
    // reference asserts against (model.py:606); the device bookkeeping has no way to report it, so refuse up front
    if (per_node_beam_size < 2) return fail(h, GITCAP_ERR_ARG, "beam_search: per_node_beam_size must be >= 2 (model.py:606)");
    if (so.n > beams * per_node_beam_size)
        return fail(h, GITCAP_ERR_ARG, "beam_search: the attached num_keep_best exceeds beams * per_node_beam_size");
    // a row must be left with per_node_beam_size columns to draw: the filter guarantees max(top_k, 2) under top_k and 2 under top_p
    if (so.smp.on && ((so.smp.top_p < 1.0f && per_node_beam_size > 2) ||
                      (so.smp.top_k > 0 && std::max(so.smp.top_k, 2) < per_node_beam_size) || per_node_beam_size > h->c.vocab_size))
        return fail(h, GITCAP_ERR_ARG, "beam_search: per_node_beam_size exceeds the columns the attached sampling filter is sure to keep");
    if (so.smp.on && h->c.vocab_size > 32768) return fail(h, GITCAP_ERR_ARG, "beam_search: sampling takes a vocabulary of at most 32768 columns");
    // (a beam row must keep at least beams * per_node_beam_size allowed columns: launch_beam_step is never handed a sentinel)
    if (int rc = cons_check(h, max_steps, beams * per_node_beam_size, "beam_search")) return rc;
    if (opts.refused) return fail(h, GITCAP_ERR_ARG, refused_message("window"));
    return body();
}

extern "C" {

int gitcap_beam_search(gitcap_t* h, const float* frames, int B, int F, int beams, int max_steps, float length_penalty,
                       int per_node_beam_size, int64_t* decoded_out, float* logprobs_out, void* stream) {
    return beam_entry(h, true, "beam_search: null handle", TAKE_BEAM | OPT_FC, 0, beams, max_steps, per_node_beam_size, decoded_out, logprobs_out, [&]() -> int {
        hipStream_t s = (hipStream_t)stream;
        if (int rc = encode_sync(h, FrameSrc{frames, nullptr, 0, 0}, B, F, nullptr, s)) return rc;
        return beam_loop(h, B, beams, max_steps, length_penalty, per_node_beam_size, decoded_out, logprobs_out, nullptr, s);
    });
}

// raw: as greedy_submit
static int beam_submit(gitcap* h, const char* null_msg, FrameSrc src, bool raw, int B, int F, float* visual_out, int beams, int max_steps,
                       float length_penalty, int per_node_beam_size, int64_t* decoded_out, float* logprobs_out, float* step_logits_out,
                       hipStream_t stream, int* ticket) {
    return beam_entry(h, ticket != nullptr, null_msg, TAKE_BEAM | OPT_FC, 0, beams, max_steps, per_node_beam_size, decoded_out, logprobs_out, [&]() -> int {
        if (int rc = raw ? check_raw(h, src.u8, B, F, src.H, src.W) : 0) return rc;
        return submit_common(h, src, B, F, visual_out, stream, ticket, [&](hipStream_t s) {
            return beam_loop(h, B, beams, max_steps, length_penalty, per_node_beam_size, decoded_out, logprobs_out, step_logits_out, s);
        });
    });
}

int gitcap_beam_search_submit(gitcap_t* h, const float* frames, int B, int F, float* visual_out, int beams, int max_steps,
                              float length_penalty, int per_node_beam_size, int64_t* decoded_out, float* logprobs_out,
                              float* step_logits_out, void* stream, int* ticket) {
    return beam_submit(h, "beam_search_submit: null argument", FrameSrc{frames, nullptr, 0, 0}, false, B, F, visual_out, beams, max_steps,
                       length_penalty, per_node_beam_size, decoded_out, logprobs_out, step_logits_out, (hipStream_t)stream, ticket);
}

int gitcap_beam_search_raw_submit(gitcap_t* h, const uint8_t* frames_hwc_bgr, int B, int F, int H, int W, float* visual_out, int beams,
                                  int max_steps, float length_penalty, int per_node_beam_size, int64_t* decoded_out,
                                  float* logprobs_out, float* step_logits_out, void* stream, int* ticket) {
    return beam_submit(h, "beam_search_raw_submit: null argument", FrameSrc{nullptr, frames_hwc_bgr, H, W}, true, B, F, visual_out, beams,
                       max_steps, length_penalty, per_node_beam_size, decoded_out, logprobs_out, step_logits_out, (hipStream_t)stream, ticket);
}

// ---- frame window ------------------------------------------------------------------------------------------------------------
// A ViT frame is encoded on its own (attention stays inside the frame, every GEMM and row kernel is batch invariant), and the only
// step between the encoder and the decoder that depends on a frame's position in the clip is the temporal embedding, added after
// ln_post in fp32.  So the ring keeps each frame's fp32 ln_post rows once, and a caption of the window adds the embedding of each
// frame's current position (window_assemble_kernel: the add of the fused epilogue) and runs the decoder's image prefix.

int gitcap_window_reset(gitcap_t* h, int B, int F) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "window_reset: null handle");
    REFUSE_FC(h, "window_reset");
    GUARD(h);
    if (B < 0 || (B > 0 && (B > h->c.max_batch || F < 1 || F > h->c.max_frames || (h->c.num_frames > 0 && F > h->c.num_frames))))
        return fail(h, GITCAP_ERR_ARG, "window_reset: B / F outside the sizes the handle was created for");
    const int64_t bytes = B > 0 ? (int64_t)B * F * h->N * h->Dv * 4 : 0;
    if (h->win_ring && bytes != h->win_bytes) {
        HIP_OK(h, hipDeviceSynchronize());        // pushes or window calls in flight may still use the ring
        HIP_OK(h, hipFree(h->win_ring));
        h->win_ring = nullptr; h->win_bytes = 0;
    }
    h->win_B = 0;
    h->win.reset(0);
    if (B == 0) return 0;
    HIP_OK(h, h->win_order.ensure());
    if (!h->win_ring) {
        hipError_t e = hipMalloc(&h->win_ring, (size_t)bytes);
        if (e != hipSuccess) { h->win_ring = nullptr; return fail(h, GITCAP_ERR_NOMEM, std::string("hipMalloc frame window: ") + hipGetErrorString(e)); }
        h->win_bytes = bytes;
    }
    h->win_B = B;
    h->win.reset(F);
    return 0;
}

// encode n new frames of each clip and append them to the ring: fp32 ln_post rows -> staging -> ring slots
static int window_push(gitcap* h, FrameSrc src, int B, int n, hipStream_t s) {
    REFUSE_FC(h, "window_push");
    if (!h->win_ring) return fail(h, GITCAP_ERR_STATE, "window_push: no frame window (gitcap_window_reset first)");
    if (B != h->win_B || n < 1 || n > h->win.slots) return fail(h, GITCAP_ERR_ARG, "window_push: B differs from the reset's, or n outside [1, F]");
    int rc = src.u8 ? check_raw(h, src.u8, B, n, src.H, src.W) : check_frames(h, src.f32, B, n);
    if (rc) return rc;
    select_slot(h, 0);
    HIP_OK(h, join_async(h, s));
    HIP_OK(h, h->win_order.before_push(s));
    HIP_OK(h, h->pool_order.before_push(s));        // (the pool's pushes and calls use the same encoder workspace; nothing without a pool)
    // staging: the q|k|v buffer of the image rows (bf16 [Mi][3 Dv], 1.5x the bytes of fp32 [Mi][Dv]) is dead once the last block's
    // attention has read it, and only the final FC2 + ln_post launch and the scatter run after that
    float* stage = (float*)h->qkv;
    if ((rc = encode_frames(h, src, B, n, stage, nullptr, false, s))) return rc;
    {
        ProfScope ps(h, GITCAP_PROF_ROWOPS, s, 0.0, 8.0 * B * n * (double)h->N * h->Dv);
        HIP_OK(h, launch_window_scatter(stage, h->win_ring, B, n, h->win.slots, h->win.head, h->N, h->Dv, s));
    }
    HIP_OK(h, h->win_order.after_push(s));
    h->win.push(n);
    return 0;
}

int gitcap_window_push(gitcap_t* h, const float* frames, int B, int n, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "window_push: null handle");
    GUARD(h);
    POLL(h);
    return window_push(h, FrameSrc{frames, nullptr, 0, 0}, B, n, (hipStream_t)stream);
}

int gitcap_window_push_raw(gitcap_t* h, const uint8_t* frames_hwc_bgr, int B, int n, int H, int W, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "window_push_raw: null handle");
    GUARD(h);
    POLL(h);
    return window_push(h, FrameSrc{nullptr, frames_hwc_bgr, H, W}, B, n, (hipStream_t)stream);
}

// the current window -> decoder input (+ visual features) -> image prefix on slot 0
static int window_prefix(gitcap* h, float* visual_out, hipStream_t s) {
    if (!h->win_ring || !h->win.full()) return fail(h, GITCAP_ERR_STATE, "window: fewer than F frames pushed since the reset");
    if (((uintptr_t)visual_out & 15) != 0) return fail(h, GITCAP_ERR_ARG, "window: visual_out must be 16-byte aligned");
    const int B = h->win_B, F = h->win.slots, N = h->N, Dv = h->Dv;
    const float* temporal = h->c.num_frames > 0 ? h->temporal : nullptr;
    select_slot(h, 0);
    HIP_OK(h, join_async(h, s));
    HIP_OK(h, h->win_order.before_read(s));
    cur(h).have = false;
    {
        const double rows = (double)B * F * N;
        ProfScope ps(h, GITCAP_PROF_ROWOPS, s, 0.0, rows * Dv * (4.0 + 2.0 + (visual_out ? 4.0 : 0.0)));
        HIP_OK(h, launch_window_assemble(h->win_ring, temporal, h->hb, visual_out, B, F, h->win.head, N, Dv, s));
    }
    int rc = image_prefix(h, B, F * N, s);
    if (rc) return rc;
    HIP_OK(h, h->win_order.after_read(s));
    return 0;
}

int gitcap_window_greedy(gitcap_t* h, int max_len, int stop, float* visual_out, int64_t* ids_out, int32_t* steps_out, void* stream) {
    return greedy_entry(h, true, "window_greedy: null handle", TAKE_GREEDY, OPT_FC, max_len, stop, ids_out, [&]() -> int {
        hipStream_t s = (hipStream_t)stream;
        if (int rc = window_prefix(h, visual_out, s)) return rc;
        return greedy_text_loop(h, h->win_B, max_len, stop, ids_out, steps_out, s);
    });
}

int gitcap_greedy_draft(gitcap_t* h, const float* frames, int B, int F, const int64_t* draft_ids, int ld_draft, int n_draft, int max_len,
                        int stop, int64_t* ids_out, int32_t* steps_out, int32_t* accepted_out, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    return greedy_draft_entry(h, "greedy_draft: null handle", OPT_LP | OPT_FC, 0, Draft{draft_ids, ld_draft, n_draft, accepted_out}, max_len, stop,
                              ids_out, steps_out, s, [&]() -> int { return encode_sync(h, FrameSrc{frames, nullptr, 0, 0}, B, F, nullptr, s); });
}

int gitcap_window_greedy_draft(gitcap_t* h, const int64_t* draft_ids, int ld_draft, int n_draft, int max_len, int stop, float* visual_out,
                               int64_t* ids_out, int32_t* steps_out, int32_t* accepted_out, void* stream) {
    hipStream_t s = (hipStream_t)stream;
    return greedy_draft_entry(h, "window_greedy_draft: null handle", OPT_LP, OPT_FC, Draft{draft_ids, ld_draft, n_draft, accepted_out}, max_len,
                              stop, ids_out, steps_out, s, [&]() -> int { return window_prefix(h, visual_out, s); });
}

int gitcap_draft_stats(const gitcap_t* h, int64_t* out4) {
    if (!h || !out4) return GITCAP_ERR_ARG;
    out4[0] = h->draft_calls; out4[1] = h->draft_offered; out4[2] = h->draft_accepted; out4[3] = h->draft_tail_steps;
    return 0;
}

int gitcap_window_beam_search(gitcap_t* h, int beams, int max_steps, float length_penalty, int per_node_beam_size,
                              float* visual_out, int64_t* decoded_out, float* logprobs_out, void* stream) {
    return beam_entry(h, true, "window_beam_search: null handle", TAKE_BEAM, OPT_FC, beams, max_steps, per_node_beam_size, decoded_out, logprobs_out, [&]() -> int {
        hipStream_t s = (hipStream_t)stream;
        if (int rc = window_prefix(h, visual_out, s)) return rc;
        return beam_loop(h, h->win_B, beams, max_steps, length_penalty, per_node_beam_size, decoded_out, logprobs_out, nullptr, s);
    });
}

// first use by gitcap_attach_token_logprobs or gitcap_score: the third head partial beside amax_val, one buffer per slot
// ---- stream pool ---------------------------------------------------------------------------------------------------------------
// The window above is ONE cursor: its clips advance in lockstep.  The pool keeps one cursor per stream over a ring of the same
// rows; a push encodes its frames as one packed pass of one-frame clips (the ragged path's encoder pass) and scatters them to ring
// frames the host planned; a pool call assembles the named streams' frames, oldest first, PACKED -- the layout of
// gitcap_attach_frame_counts -- and runs the image prefix and the token loop of that call.

int gitcap_pool_reset(gitcap_t* h, int n_streams, int F) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "pool_reset: null handle");
    REFUSE_FC(h, "pool_reset");
    GUARD(h);
    if (n_streams < 0 || n_streams > 4096) return fail(h, GITCAP_ERR_ARG, "pool_reset: n_streams outside 0..4096");
    if (n_streams > 0 && (F < 1 || F > 255 || F > h->c.max_frames || (h->c.num_frames > 0 && F > h->c.num_frames)))
        return fail(h, GITCAP_ERR_ARG, "pool_reset: F outside the sizes the handle was created for");
    const int64_t ring_bytes = n_streams > 0 ? (int64_t)n_streams * F * h->N * h->Dv * 4 : 0;
    if (ring_bytes > ((int64_t)8 << 30)) return fail(h, GITCAP_ERR_ARG, "pool_reset: the ring (n_streams * F * tokens * enc_width * 4 bytes) would exceed 8 GiB");
    if (n_streams > 0 && !h->finalized) return fail(h, GITCAP_ERR_STATE, "pool_reset: weights not finalized");
    if (h->pool_ring && (n_streams != h->pool_S || F != h->pool_F)) {
        HIP_OK(h, hipDeviceSynchronize());          // pushes or pool calls in flight may still use the buffers
        pool_free(h);
    }
    if (n_streams == 0) return 0;
    if (!h->pool_ring) {
        const size_t cap = (size_t)h->c.max_batch * h->c.max_frames;
        HIP_OK(h, h->pool_order.ensure());
        hipError_t e = hipMalloc((void**)&h->pool_ring, (size_t)ring_bytes);
        if (e == hipSuccess) e = hipMalloc((void**)&h->pool_tab, 3 * cap * sizeof(int32_t));
        if (e == hipSuccess) e = h->pool_push_host.ensure(cap);
        if (e == hipSuccess) e = h->pool_call_host.ensure(2 * cap);
        if (e != hipSuccess) {
            pool_free(h);
            return fail(h, GITCAP_ERR_NOMEM, std::string("hipMalloc stream pool: ") + hipGetErrorString(e));
        }
        h->pool_bytes = ring_bytes + (int64_t)(3 * cap * sizeof(int32_t));
        h->pool_S = n_streams; h->pool_F = F; h->pool_cap = (int)cap;
        h->pool.resize((size_t)n_streams);
    }
    for (RingCursor& c : h->pool) c.reset(F);
    return 0;
}

// the message of a plan the host refused (host_logic.h: pool_plan); unit = "frame" (a push) or "row" (a pool call)
static std::string pool_refused(const gitcap* h, const char* who, const char* unit, int why, int bad, int32_t id) {
    const std::string head = std::string(who) + ": " + unit + " " + std::to_string(bad);
    switch (why) {
        case POOL_PLAN_BAD_ID: return head + " names stream " + std::to_string(id) + ", outside [0, " + std::to_string(h->pool_S) + ")";
        case POOL_PLAN_OVER: return head + " is more than F = " + std::to_string(h->pool_F) + " for stream " + std::to_string(id) + " in one push";
        case POOL_PLAN_TWICE: return std::string(who) + ": stream " + std::to_string(id) + " is named twice";
        default: return std::string(who) + ": stream " + std::to_string(id) + " holds no frame";
    }
}

// encode the n frames as n one-frame clips (no temporal add) and copy each to the ring frame the plan gave it
static int pool_push(gitcap* h, const char* who, FrameSrc src, const int32_t* stream_ids, int n, hipStream_t s) {
    REFUSE_FC(h, who);
    const std::string w(who);
    if (!h->pool_ring) return fail(h, GITCAP_ERR_STATE, w + ": no pool (gitcap_pool_reset first)");
    if (!stream_ids) return fail(h, GITCAP_ERR_ARG, w + ": null stream_ids");
    if (n < 1 || n > h->pool_cap) return fail(h, GITCAP_ERR_ARG, w + ": n outside [1, max_batch * max_frames = " + std::to_string(h->pool_cap) + "]");
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "weights not finalized");
    if (!src.u8 && !src.f32) return fail(h, GITCAP_ERR_ARG, w + ": null frames");
    if (src.u8 ? (src.H <= 0 || src.W <= 0 || (int64_t)n * src.H * src.W * 3 > ((int64_t)1 << 40)) : ((uintptr_t)src.f32 & 15) != 0)
        return fail(h, GITCAP_ERR_ARG, w + ": empty or oversized camera frames, or fp32 frames not 16-byte aligned");
    std::vector<RingCursor> after = h->pool;
    std::vector<int32_t> dst((size_t)n);
    PoolPlan plan;
    int bad = -1;
    if (const int why = pool_plan(after, stream_ids, n, dst.data(), nullptr, 0, nullptr, nullptr, nullptr, nullptr, &plan, &bad))
        return fail(h, GITCAP_ERR_ARG, pool_refused(h, who, "frame", why, bad, stream_ids[bad]));
    select_slot(h, 0);
    HIP_OK(h, h->pool_push_host.wait());
    memcpy(h->pool_push_host.p, dst.data(), (size_t)n * sizeof(int32_t));
    HIP_OK(h, join_async(h, s));
    HIP_OK(h, h->pool_order.before_push(s));
    HIP_OK(h, h->win_order.before_push(s));         // (the window's pushes and calls use the same encoder workspace)
    // From here on ring frames may be half written: a failure empties the streams this push names.
    auto enqueue = [&]() -> int {
        HIP_OK(h, h->pool_push_host.copy(h->pool_tab, 0, (size_t)n, s));
        HIP_OK(h, h->pool_push_host.mark(s));
        float* stage = (float*)h->qkv;              // window_push's staging: dead behind the last block's attention
        if (int rc = encode_frames(h, src, n, 1, stage, nullptr, false, s)) return rc;
        ProfScope ps(h, GITCAP_PROF_ROWOPS, s, 0.0, 8.0 * n * (double)h->N * h->Dv);
        HIP_OK(h, launch_pool_scatter(PoolScatterArgs{stage, h->pool_ring, h->pool_tab, n, h->N, h->Dv}, s));
        return 0;
    };
    int rc = enqueue();
    if (!rc) {
        const hipError_t e = h->pool_order.after_push(s);
        if (e != hipSuccess) rc = fail(h, GITCAP_ERR_HIP, std::string("pool push: ") + hipGetErrorString(e));
    }
    if (rc) {
        for (int i = 0; i < n; ++i) h->pool[(size_t)stream_ids[i]].reset(h->pool_F);
        return rc;
    }
    h->pool.swap(after);
    return 0;
}

int gitcap_pool_push(gitcap_t* h, const float* frames, const int32_t* stream_ids, int n, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "pool_push: null handle");
    GUARD(h);
    POLL(h);
    return pool_push(h, "pool_push", FrameSrc{frames, nullptr, 0, 0}, stream_ids, n, (hipStream_t)stream);
}

int gitcap_pool_push_raw(gitcap_t* h, const uint8_t* frames_hwc_bgr, const int32_t* stream_ids, int n, int H, int W, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "pool_push_raw: null handle");
    GUARD(h);
    POLL(h);
    if (!frames_hwc_bgr) return fail(h, GITCAP_ERR_ARG, "pool_push_raw: null frames");
    return pool_push(h, "pool_push_raw", FrameSrc{nullptr, frames_hwc_bgr, H, W}, stream_ids, n, (hipStream_t)stream);
}

// the named streams' frames -> decoder input -> image prefix on slot 0; frames_out (host, nullable) = the frames each row saw
static int pool_prefix(gitcap* h, const char* who, const int32_t* stream_ids, int B, int32_t* frames_out, hipStream_t s) {
    const std::string w(who);
    if (!h->pool_ring) return fail(h, GITCAP_ERR_STATE, w + ": no pool (gitcap_pool_reset first)");
    if (!stream_ids || B < 1 || B > h->c.max_batch || B > 256) return fail(h, GITCAP_ERR_ARG, w + ": null stream_ids, or B outside [1, min(max_batch, 256)]");
    const int N = h->N, cap = h->pool_cap;
    std::vector<RingCursor> cursors = h->pool;
    std::vector<int32_t> tab((size_t)B * h->pool_F * 2 + 2 * (size_t)B);
    int32_t *src = tab.data(), *pos = src + (size_t)B * h->pool_F, *off = pos + (size_t)B * h->pool_F, *len = off + B;
    PoolPlan plan;
    int bad = -1;
    if (const int why = pool_plan(cursors, nullptr, 0, nullptr, stream_ids, B, src, pos, off, len, &plan, &bad))
        return fail(h, why == POOL_PLAN_EMPTY ? GITCAP_ERR_STATE : GITCAP_ERR_ARG, pool_refused(h, who, "row", why, bad, stream_ids[bad]));
    if (plan.total > cap) return fail(h, GITCAP_ERR_ARG, w + ": the named streams hold more than max_batch * max_frames frames");
    select_slot(h, 0);
    HIP_OK(h, h->pool_call_host.wait());
    memcpy(h->pool_call_host.p, src, (size_t)plan.total * sizeof(int32_t));
    memcpy(h->pool_call_host.p + cap, pos, (size_t)plan.total * sizeof(int32_t));
    HIP_OK(h, join_async(h, s));
    HIP_OK(h, h->pool_order.before_read(s));
    cur(h).have = false;
    int32_t *d_src = h->pool_tab + cap, *d_pos = h->pool_tab + 2 * (size_t)cap;
    HIP_OK(h, h->pool_call_host.copy(d_src, 0, (size_t)plan.total, s));
    HIP_OK(h, h->pool_call_host.copy(d_pos, (size_t)cap, (size_t)plan.total, s));
    HIP_OK(h, h->pool_call_host.mark(s));
    {
        ProfScope ps(h, GITCAP_PROF_ROWOPS, s, 0.0, (double)plan.total * N * h->Dv * (4.0 + 2.0));
        HIP_OK(h, launch_pool_assemble(PoolAssembleArgs{h->pool_ring, h->c.num_frames > 0 ? h->temporal : nullptr, d_src, d_pos, h->hb,
                                                        plan.total, N, h->Dv}, s));
    }
    int rc;
    if (plan.dense) {
        rc = image_prefix(h, B, plan.maxn * N, s);          // equal counts: the dense layout [B][n][N][Dv], launch for launch
    } else {
        RaggedCounts& fc = h->call.fc;                       // (image_prefix reads the counts; the entry's CallScope empties them)
        fc.B = B;
        for (int r = 0; r < B; ++r) fc.n[r] = (unsigned char)len[r];
        gitcap::Slot& sl = cur(h);
        HIP_OK(h, launch_ragged_tables(fc, N, sl.off, sl.len, sl.fpos, s));
        rc = image_prefix(h, B, plan.maxn * N, s, plan.total * N);
    }
    if (rc) return rc;
    HIP_OK(h, h->pool_order.after_read(s));
    if (frames_out)
        for (int r = 0; r < B; ++r) frames_out[r] = len[r];
    return 0;
}

int gitcap_pool_greedy(gitcap_t* h, const int32_t* stream_ids, int B, int max_len, int stop, int64_t* ids_out, int32_t* steps_out,
                       int32_t* frames_out, void* stream) {
    return greedy_entry(h, true, "pool_greedy: null handle", TAKE_GREEDY, OPT_FC, max_len, stop, ids_out, [&]() -> int {
        hipStream_t s = (hipStream_t)stream;
        if (int rc = pool_prefix(h, "pool_greedy", stream_ids, B, frames_out, s)) return rc;
        return greedy_text_loop(h, B, max_len, stop, ids_out, steps_out, s);
    });
}

int gitcap_pool_beam_search(gitcap_t* h, const int32_t* stream_ids, int B, int beams, int max_steps, float length_penalty,
                            int per_node_beam_size, int64_t* decoded_out, float* logprobs_out, void* stream) {
    return beam_entry(h, true, "pool_beam_search: null handle", TAKE_BEAM, OPT_FC, beams, max_steps, per_node_beam_size, decoded_out, logprobs_out, [&]() -> int {
        hipStream_t s = (hipStream_t)stream;
        if (int rc = pool_prefix(h, "pool_beam_search", stream_ids, B, nullptr, s)) return rc;
        return beam_loop(h, B, beams, max_steps, length_penalty, per_node_beam_size, decoded_out, logprobs_out, nullptr, s);
    });
}

int gitcap_pool_drop(gitcap_t* h, int stream_id) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "pool_drop: null handle");
    if (!h->pool_ring) return fail(h, GITCAP_ERR_STATE, "pool_drop: no pool (gitcap_pool_reset first)");
    if (stream_id < 0 || stream_id >= h->pool_S) return fail(h, GITCAP_ERR_ARG, "pool_drop: stream outside the pool");
    h->pool[(size_t)stream_id].reset(h->pool_F);     // (what is in flight was enqueued with the old cursor; pool_order orders the next push)
    return 0;
}

int gitcap_pool_counts(const gitcap_t* h, int32_t* counts_out) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "pool_counts: null handle");
    if (!counts_out) return fail(h, GITCAP_ERR_ARG, "pool_counts: null counts_out");
    if (!h->pool_ring) return fail(h, GITCAP_ERR_STATE, "pool_counts: no pool (gitcap_pool_reset first)");
    for (int i = 0; i < h->pool_S; ++i) counts_out[i] = h->pool[(size_t)i].count;
    return 0;
}

static int ensure_amax_sum(gitcap* h) {
    if (h->slots[0].amax_sum) return 0;
    for (auto& sl : h->slots)
        if (int rc = dev_alloc(h, &sl.amax_sum, (size_t)sl.Mt * (size_t)((h->V + 15) / 16))) { h->slots[0].amax_sum = nullptr; return rc; }
    return 0;
}

int gitcap_attach_token_logprobs(gitcap_t* h, float* logprobs_out, int ld) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "attach_token_logprobs: null handle");
    if (!logprobs_out) { h->pending.lp = LpAttach{}; return 0; }
    if (ld < 1 || ((uintptr_t)logprobs_out & 3) != 0) return fail(h, GITCAP_ERR_ARG, "attach_token_logprobs: ld < 1 or a misaligned pointer");
    GUARD(h);
    if (int rc = ensure_amax_sum(h)) return rc;
    h->pending.lp = LpAttach{logprobs_out, ld};
    return 0;
}

int gitcap_attach_top_logprobs(gitcap_t* h, int k, int64_t* top_ids, float* top_lp, int ld) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "attach_top_logprobs: null handle");
    if (k == 0 || !top_ids || !top_lp) { h->pending.tk = TopkAttach{}; return 0; }
    if (const char* bad = tk_attach_bad(k, top_ids, top_lp, ld)) return fail(h, GITCAP_ERR_ARG, std::string("attach_top_logprobs: ") + bad);
    if (!head_topk_ok(h->c.dec_width, h->head_w.scale != nullptr)) return fail(h, GITCAP_ERR_ARG, "attach_top_logprobs: no top-k kernel for this decoder width");
    GUARD(h);
    if (int rc = ensure_amax_sum(h)) return rc;             // the head's third partial, per slot: all the feature allocates
    h->pending.tk = TopkAttach{k, top_ids, top_lp, ld};
    return 0;
}

int gitcap_score(gitcap_t* h, const int64_t* ids, int ld_ids, int rows, int beams, int T, const int32_t* lengths, int64_t ignore_id,
                 float* token_lp, int ld_lp, float* row_sum, int32_t* row_cnt, int64_t* top1_ids, float* top1_lp, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "score: null handle");
    CallScope opts(h->pending, h->call, OPT_TK, 0);         // the top-k attachment is consumed, whatever becomes of the call
    if (int rc = tk_check(h, "score", h->call.tk, T - 1)) return rc;
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "score: weights not finalized");
    if (!h->slots[0].have) return fail(h, GITCAP_ERR_STATE, "score before encode/set_visual");
    if (T < 2 || ld_ids < T) return fail(h, GITCAP_ERR_ARG, "score: T < 2 (CLS and at least one token) or ld_ids < T");
    if (token_lp && ld_lp < T - 1) return fail(h, GITCAP_ERR_ARG, "score: ld_lp < T - 1");
    GUARD(h);
    POLL(h);
    select_slot(h, 0);
    gitcap::Slot& sl = cur(h);
    int rc;
    if ((rc = ensure_amax_sum(h))) return rc;
    if (!sl.score_buf && (rc = dev_alloc(h, &sl.score_buf, 2 * (size_t)sl.Mt))) return rc;
    HIP_OK(h, join_async(h, (hipStream_t)stream));
    const ScoreReq sq{lengths, ignore_id, token_lp, ld_lp, row_sum, row_cnt, top1_ids, top1_lp, h->call.tk};
    TextReq q;
    q.ids = ids; q.ld_ids = ld_ids; q.rows = rows; q.beams = beams; q.T = T; q.score = &sq;
    return text_forward(h, q, (hipStream_t)stream);
}

int gitcap_dbg_score_target_logits(gitcap_t* h, float* out, int n, void* stream) {
    if (!h || !out || n <= 0) return fail(h, GITCAP_ERR_ARG, "dbg_score_target_logits: null argument");
    if (!h->slots[0].score_buf || n > h->slots[0].Mt) return fail(h, GITCAP_ERR_STATE, "dbg_score_target_logits: no gitcap_score call yet, or n beyond the workspace");
    GUARD(h);
    HIP_OK(h, hipMemcpyAsync(out, h->slots[0].score_buf, (size_t)n * 4, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// first gitcap_distill: the partial buffers (nothing is kept of a failed attempt but what the handle frees anyway)
static int ensure_distill(gitcap* h) {
    gitcap::Distill& d = h->dist;
    if (d.rows) return 0;
    const size_t n = (size_t)h->slots[0].Mt * (size_t)((h->V + 15) / 16);
    int rc;
    if ((rc = dev_alloc(h, &d.t_max, n)) || (rc = dev_alloc(h, &d.t_idx, n)) || (rc = dev_alloc(h, &d.t_sum, n)) || (rc = dev_alloc(h, &d.s_max, n)) ||
        (rc = dev_alloc(h, &d.s_idx, n)) || (rc = dev_alloc(h, &d.s_sum, n)) || (rc = dev_alloc(h, &d.cross, n)))
        return rc;
    return dev_alloc(h, &d.rows, 2 * (size_t)h->slots[0].Mt);
}

int gitcap_distill(gitcap_t* h, gitcap_student_t* st, const int64_t* ids, int ld_ids, int rows, int beams, int T, const int32_t* lengths,
                   int64_t ignore_id, float temperature, const gitcap_distill_out* out, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "distill: null teacher handle");
    if (!st) return fail(h, GITCAP_ERR_ARG, "distill: null student handle");
    if (!ids || !out || !out->kl) return fail(h, GITCAP_ERR_ARG, "distill: null ids, out or out->kl");
    if (!h->finalized) return fail(h, GITCAP_ERR_STATE, "distill: teacher weights not finalized");
    if (!h->slots[0].have) return fail(h, GITCAP_ERR_STATE, "distill before encode/set_visual");
    if (!(temperature > 0.f) || !std::isfinite(temperature)) return fail(h, GITCAP_ERR_ARG, "distill: temperature must be positive and finite");
    if (T < 1 || ld_ids < T || out->ld_kl < T) return fail(h, GITCAP_ERR_ARG, "distill: T < 1, ld_ids < T or ld_kl < T");
    if ((out->teacher_lp || out->student_lp) && out->ld_lp < T - 1) return fail(h, GITCAP_ERR_ARG, "distill: ld_lp < T - 1");
    if (rows <= 0 || beams <= 0 || rows != h->slots[0].B * beams || rows > h->R) return fail(h, GITCAP_ERR_ARG, "distill: rows != encoded clips * beams, or beyond max_batch*max_beams");
    if (T > h->Tmax || T > h->c.max_text_pos || (int64_t)rows * T > h->slots[0].Mt) return fail(h, GITCAP_ERR_ARG, "distill: T exceeds max_text_len / max_text_pos");
    if (student_device(st) != h->device) return fail(h, GITCAP_ERR_ARG, "distill: the two handles live on different devices");
    std::string why;
    if (int rc = student_rows_check(st, rows, T, why)) return fail(h, rc, "distill: " + why);
    const HeadWeight sw = student_head_weight(st);
    if (sw.V != h->V) return fail(h, GITCAP_ERR_ARG, "distill: the two models' vocab_size differ");
    if (!head_dual_ok(h->D, sw.D)) return fail(h, GITCAP_ERR_ARG, "distill: no dual head for these two widths");
    const float inv_temp = 1.0f / temperature;
    if (!(inv_temp > 0.f) || !std::isfinite(inv_temp)) return fail(h, GITCAP_ERR_ARG, "distill: 1 / temperature is not a positive finite fp32");
    GUARD(h);
    POLL(h);
    select_slot(h, 0);
    gitcap::Slot& sl = cur(h);
    int rc;
    if ((rc = ensure_distill(h))) return rc;
    hipStream_t s = (hipStream_t)stream;
    HIP_OK(h, join_async(h, s));
    // both stacks up to their final LayerNorm rows (the "rows only, no head" request of the existing passes), then the two launches
    TextReq q;
    q.ids = ids; q.ld_ids = ld_ids; q.rows = rows; q.beams = beams; q.T = T;
    if ((rc = text_forward(h, q, s))) return rc;
    StudentRows sr{};
    if ((rc = student_forward_rows(st, ids, ld_ids, rows, T, s, &sr, why))) return fail(h, rc, "distill: " + why);
    const gitcap::Distill& d = h->dist;
    const int M = rows * T, V = h->V;
    const bool want_lp = out->teacher_lp || out->student_lp;
    DualHeadArgs da{};
    da.Xt = sl.xsb; da.ldxt = h->D; da.Xs = sr.xb; da.ldxs = sr.head.D;
    da.wt = HeadWeight{h->head_w.p, h->head_w.pk, h->head_w.scale, h->head_b, V, h->D}; da.ws = sr.head;
    da.M = M; da.inv_temp = inv_temp;
    da.t_max = d.t_max; da.t_idx = d.t_idx; da.t_sum = d.t_sum; da.s_max = d.s_max; da.s_idx = d.s_idx; da.s_sum = d.s_sum; da.cross = d.cross;
    if (want_lp) { da.tg = HeadTargets{ids, T, ld_ids, 1, d.rows}; da.s_logit = d.rows + sl.Mt; }
    {
        ProfScope ps(h, GITCAP_PROF_SKINNY, s, 2.0 * M * V * (h->D + sr.head.D), (h->head_w.scale ? 1.0 : 2.0) * V * h->D + 2.0 * V * sr.head.D);
        HIP_OK(h, launch_head_dual(da, s));
    }
    const DistillOut o{out->kl, out->ld_kl, out->teacher_top1, out->student_top1, out->agree, out->teacher_lp, out->student_lp, out->ld_lp,
                       out->row_kl_sum, out->row_cnt};
    HIP_OK(h, launch_distill_final(DistillPartials{d.t_max, d.t_idx, d.t_sum, d.s_max, d.s_idx, d.s_sum, d.cross}, (V + 15) / 16, d.rows,
                                   d.rows + sl.Mt, ids, ld_ids, rows, T, lengths, ignore_id, V, o, s));
    return 0;
}

int gitcap_attach_prompt(gitcap_t* h, const int64_t* prompt_ids, int ld, const int32_t* lengths, int min_len, int max_len) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "attach_prompt: null handle");
    h->pending.pr = PromptArgs{};
    if (!prompt_ids && !lengths) return 0;                   // detach
    if (!prompt_ids || !lengths) return fail(h, GITCAP_ERR_ARG, "attach_prompt: prompt_ids and lengths are both required");
    if (((uintptr_t)prompt_ids & 7) != 0 || ((uintptr_t)lengths & 3) != 0) return fail(h, GITCAP_ERR_ARG, "attach_prompt: a misaligned pointer");
    if (min_len < 1 || max_len < min_len || ld < max_len) return fail(h, GITCAP_ERR_ARG, "attach_prompt: need 1 <= min_len <= max_len <= ld");
    h->pending.pr = PromptArgs{prompt_ids, ld, lengths, min_len, max_len};
    return 0;
}

int gitcap_attach_frame_counts(gitcap_t* h, const int32_t* counts, int B) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "attach_frame_counts: null handle");
    h->pending.fc.B = 0;
    if (!counts) return 0;                                   // detach
    if (B < 1 || B > h->c.max_batch || B > 256) return fail(h, GITCAP_ERR_ARG, "attach_frame_counts: B outside [1, min(max_batch, 256)]");
    const int limit = std::min(255, h->c.num_frames > 0 ? std::min(h->c.max_frames, h->c.num_frames) : h->c.max_frames);
    int64_t total = 0;
    for (int b = 0; b < B; ++b) {
        if (counts[b] < 1 || counts[b] > limit)
            return fail(h, GITCAP_ERR_ARG, "attach_frame_counts: clip " + std::to_string(b) + " has " + std::to_string(counts[b]) +
                        " frames, outside [1, " + std::to_string(limit) + "]");
        total += counts[b];
    }
    if (total > (int64_t)h->c.max_batch * h->c.max_frames) return fail(h, GITCAP_ERR_ARG, "attach_frame_counts: the counts sum beyond max_batch * max_frames");
    for (int b = 0; b < B; ++b) h->pending.fc.n[b] = (unsigned char)counts[b];
    h->pending.fc.B = B;
    return 0;
}

int gitcap_attach_constraints(gitcap_t* h, const gitcap_constraints* c) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "attach_constraints: null handle");
    h->pending.co = ConsOpt{};
    if (!c) return 0;                                        // detach
    if (c->no_repeat_ngram_size < 0 || c->min_length < 0 || c->n_suppress < 0) return fail(h, GITCAP_ERR_ARG, "attach_constraints: a negative field");
    if (c->n_suppress > 256) return fail(h, GITCAP_ERR_ARG, "attach_constraints: n_suppress > 256");
    if (c->n_suppress > 0 && (!c->suppress || ((uintptr_t)c->suppress & 3) != 0))
        return fail(h, GITCAP_ERR_ARG, "attach_constraints: n_suppress > 0 with a null or misaligned suppress pointer");
    if (h->c.vocab_size > 131072) return fail(h, GITCAP_ERR_ARG, "attach_constraints: the ban mask takes a vocabulary of at most 131072 columns");
    GUARD(h);
    if (!h->slots[0].ban_mask) {                             // first attach: one mask per pipeline slot, rows x ld (ld even, >= ceil(V / 16))
        h->ban_ld = (((h->V + 15) / 16) + 1) & ~1;
        for (auto& sl : h->slots)
            if (int rc = dev_alloc(h, &sl.ban_mask, (size_t)h->R * (size_t)h->ban_ld)) { h->slots[0].ban_mask = nullptr; return rc; }
    }
    h->pending.co = ConsOpt{true, c->no_repeat_ngram_size, c->min_length, c->n_suppress ? c->suppress : nullptr, c->n_suppress};
    return 0;
}

int gitcap_attach_search_options(gitcap_t* h, const gitcap_search_options* opt) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "attach_search_options: null handle");
    const SampleOpt smp = h->pending.so.smp;                 // a pending gitcap_attach_sampling stays pending
    if (!opt) { h->pending.so = SearchOpt{}; h->pending.so.smp = smp; return 0; }
    if (opt->num_keep_best < 1 || opt->num_keep_best > 16)
        return fail(h, GITCAP_ERR_ARG, "attach_search_options: num_keep_best outside [1, 16]");
    if (!(opt->repetition_penalty > 0.f) || !std::isfinite(opt->repetition_penalty))
        return fail(h, GITCAP_ERR_ARG, "attach_search_options: repetition_penalty must be finite and > 0");
    if (opt->num_keep_best > 1 && (!opt->nbest_out || !opt->nbest_logprobs_out))
        return fail(h, GITCAP_ERR_ARG, "attach_search_options: num_keep_best > 1 needs nbest_out and nbest_logprobs_out");
    if (((uintptr_t)opt->nbest_out & 7) != 0 || ((uintptr_t)opt->nbest_logprobs_out & 3) != 0)
        return fail(h, GITCAP_ERR_ARG, "attach_search_options: a misaligned output pointer");
    GUARD(h);
    if (opt->num_keep_best > 1 && !h->slots[0].nb_len) {     // first n-best attach: the hypothesis state of every pipeline slot
        const size_t Bm = (size_t)h->c.max_batch, T = (size_t)h->Tmax + 1;
        for (auto& sl : h->slots) {
            int rc = dev_alloc(h, &sl.nb_ids, Bm * 16 * T);
            rc = rc ? rc : dev_alloc(h, &sl.nb_score, Bm * 16);
            rc = rc ? rc : dev_alloc(h, &sl.nb_len, Bm * 16);
            if (rc) { h->slots[0].nb_len = nullptr; return rc; }
        }
    }
    h->pending.so = SearchOpt{opt->num_keep_best, opt->repetition_penalty, opt->nbest_out, opt->nbest_logprobs_out, smp};
    return 0;
}

int gitcap_attach_sampling(gitcap_t* h, const gitcap_sampling_options* opt) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "attach_sampling: null handle");
    if (!opt) { h->pending.so.smp = SampleOpt{}; return 0; }
    if (!(opt->temperature > 0.f) || !std::isfinite(opt->temperature))
        return fail(h, GITCAP_ERR_ARG, "attach_sampling: temperature must be finite and > 0");
    if (opt->top_k < 0) return fail(h, GITCAP_ERR_ARG, "attach_sampling: top_k must be >= 0");
    if (!(opt->top_p > 0.f) || !(opt->top_p <= 1.0f)) return fail(h, GITCAP_ERR_ARG, "attach_sampling: top_p outside (0, 1]");
    h->pending.so.smp = SampleOpt{true, opt->temperature, opt->top_k, opt->top_p, opt->seed};
    return 0;
}

int gitcap_reorder_rows(gitcap_t* h, const int32_t* src_rows, int rows, int t_len, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "reorder_rows: null handle");
    GUARD(h);
    POLL(h);
    if (!src_rows || rows <= 0 || rows > h->R || t_len < 0 || t_len > h->Tmax)
        return fail(h, GITCAP_ERR_ARG, "reorder_rows: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    gitcap::Slot& sl = cur(h);       // slot 0: every submission leaves it selected
    HIP_OK(h, join_async(h, s));
    HIP_OK(h, launch_gather_txt_rows(sl.kv_txt, sl.kv_txt2, src_rows, rows, t_len, h->Tmax, 3 * h->D, h->c.dec_layers,
                                     (size_t)h->R * h->Tmax * 3 * h->D, s));
    std::swap(sl.kv_txt, sl.kv_txt2);
    h->att.permuted = true;
    return 0;
}

// The maps of the text pass the handle ran last (attnmap.hip): two launches over the slot's cached q | k, nothing recomputed.
int gitcap_attention_map(gitcap_t* h, int rows, int T, int layer, const int32_t* lengths, float* frame_mass, int ld_f, float* text_mass,
                         float* patch_map, int ld_s, void* stream) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "attention_map: null handle");
    GUARD(h);
    POLL(h);
    select_slot(h, 0);
    gitcap::Slot& sl = cur(h);
    const gitcap::AttnPass& ap = h->att;
    if (!h->finalized || !sl.have || ap.T == 0)
        return fail(h, GITCAP_ERR_STATE, "attention_map: no synchronous text pass (greedy, score, text_forward) since the last image pass");
    if (ap.permuted) return fail(h, GITCAP_ERR_STATE, "attention_map: the last text pass was a beam search (its rows are permuted): score the predictions, then ask");
    if (!frame_mass || !text_mass || rows <= 0 || T <= 0) return fail(h, GITCAP_ERR_ARG, "attention_map: bad arguments");
    if (rows != ap.rows) return fail(h, GITCAP_ERR_ARG, "attention_map: rows != the rows of the last text pass");
    if (T > ap.T) return fail(h, GITCAP_ERR_STATE, "attention_map: T exceeds the positions the last text pass filled");
    if (layer < -1 || layer >= h->c.dec_layers) return fail(h, GITCAP_ERR_ARG, "attention_map: layer outside [-1, dec_layers)");
    if (h->N <= 0 || sl.S % h->N != 0) return fail(h, GITCAP_ERR_STATE, "attention_map: the image prefix is not whole frames (set_visual with another token count)");
    if (ld_f < sl.S / h->N || (patch_map && ld_s < sl.S)) return fail(h, GITCAP_ERR_ARG, "attention_map: ld_f < frames or ld_s < image tokens of the longest clip");
    if ((((uintptr_t)lengths | (uintptr_t)frame_mass | (uintptr_t)text_mass | (uintptr_t)patch_map) & 3) != 0)
        return fail(h, GITCAP_ERR_ARG, "attention_map: misaligned pointer");
    hipStream_t s = (hipStream_t)stream;
    HIP_OK(h, join_async(h, s));
    if (!h->att_stats)
        if (int rc = dev_alloc(h, &h->att_stats, attn_map_scratch_floats(h->c.dec_layers, h->c.dec_heads, h->R, h->Tmax, -1))) return rc;
    AttnMapArgs a{};
    a.kv_img = sl.kv_img; a.img_layer_stride = (size_t)h->Mi * 3 * h->D;
    a.kv_txt = sl.kv_txt; a.txt_layer_stride = (size_t)h->R * h->Tmax * 3 * h->D;
    a.L = h->c.dec_layers; a.H = h->c.dec_heads; a.D = h->D; a.rows = rows; a.rows_per_clip = ap.rows_per_clip; a.T = T; a.Tmax = h->Tmax;
    a.N = h->N; a.S_img = sl.S; a.Smax = sl.S;
    if (sl.ragged) { a.off = sl.off; a.len = sl.len; }
    a.layer = layer; a.lengths = lengths; a.stats = h->att_stats;
    a.frame_mass = frame_mass; a.ld_f = ld_f; a.text_mass = text_mass; a.patch_map = patch_map; a.ld_s = ld_s;
    HIP_OK(h, launch_attn_map(a, s));
    return 0;
}

int gitcap_poll_errors(gitcap_t* h) {
    if (!h) return GITCAP_ERR_ARG;
    GUARD(h);
    return poll_exchange(h);
}

int gitcap_profile_enable(gitcap_t* h, int enable) {
    if (!h) return GITCAP_ERR_ARG;
    h->prof_on = enable != 0;
    return 0;
}

int gitcap_profile_read(gitcap_t* h, int cls, double* ms_total, int64_t* launches, double* flops_total,
                        double* bytes_total) {
    if (!h || cls < 0 || cls >= GITCAP_PROF_CLASSES) return fail(h, GITCAP_ERR_ARG, "profile_read: bad class");
    gitcap::ProfClass& pc = h->prof[cls];
    double ms = 0, fl = 0, by = 0;
    for (size_t i = 0; i < pc.used; ++i) {
        HIP_OK(h, hipEventSynchronize(pc.recs[i].b));
        float t = 0;
        HIP_OK(h, hipEventElapsedTime(&t, pc.recs[i].a, pc.recs[i].b));
        ms += t; fl += pc.recs[i].flops; by += pc.recs[i].bytes;
    }
    if (ms_total) *ms_total = ms;
    if (launches) *launches = (int64_t)pc.used;
    if (flops_total) *flops_total = fl;
    if (bytes_total) *bytes_total = by;
    pc.used = 0;
    return 0;
}

int gitcap_preprocess(const uint8_t* frames_hwc_bgr, int nf, int H, int W, float* out_nchw, int crop, void* stream) {
    if (!frames_hwc_bgr || !out_nchw) return GITCAP_ERR_ARG;
    hipError_t e = launch_preprocess(frames_hwc_bgr, out_nchw, nf, H, W, crop, (hipStream_t)stream);
    return e == hipSuccess ? 0 : (e == hipErrorInvalidValue ? GITCAP_ERR_ARG : GITCAP_ERR_HIP);
}

// Speed-only switches at run time (the same ones the GITCAP_* environment variables set once per process): lets ONE process
// check that results do not depend on them.  key 0: GEMM + LayerNorm epilogue on/off, 1: one/two-row prologue on/off,
// 2: 256-tile threshold (GITCAP_GEMM_SMALL_TILES), 3: 128-tile threshold (GITCAP_GEMM_TINY_TILES), 4: retired (no effect),
// 5: greedy loop chains token steps (the arg-max launch embeds the next step's input rows) on/off,
// 6: polls a fused GEMM + LayerNorm tile waits for its siblings before it gives up (0 = default; 1 forces the fail-soft path),
// 7: text rows' FC1 -> GELU -> FC2 as one launch over hidden slices (ffn_txt.hip) on/off,
// 8: gitcap_finalize_weights makes fragment-major copies of the text-path weights on/off (takes effect at the next finalize),
// 9: text attention launches of more units than CUs use 8-wave workgroups (two units per CU) on/off,
// 10 / 11 / 20: see include/gitcap.h.
// Returns the old value.
int gitcap_dbg_config(int key, int value) {
    int old = -1;
    switch (key) {
        case 0: old = g_fuse_ln.exchange(value != 0); break;
        case 1: old = g_row_prologue.exchange(value != 0); break;
        case 2: old = g_small_tiles.exchange(value); break;
        case 3: old = g_tiny_tiles.exchange(value); break;
        case 4: old = 0; break;                                   // (retired: 224-row GEMM tiles for synchronous calls)
        case 5: old = g_chain_steps.exchange(value != 0); break;
        case 6: old = (int)g_ln_spin_limit.exchange((unsigned)(value > 0 ? value : 0)); break;
        case 7: old = g_ffn_fuse.exchange(value != 0); break;
        case 8: old = g_wpack.exchange(value != 0); break;
        case 9: old = g_txt8.exchange(value != 0); break;
        case 10: old = g_head_share.exchange(value != 0); break;
        case 11: old = g_rows3.exchange(value != 0); break;
        case 20: old = g_prompt_prefill.exchange(value != 0); break;     // (12 .. 19 stay unknown keys)
        default: return GITCAP_ERR_ARG;
    }
    return old;
}

// Threads a host-side copy may use: the affinity mask capped by the cgroup CPU quota (a 1-GPU box gives the job a share of the
// host: a pool as wide as the machine only time-slices against itself), at most 8 (a copy is memory bound long before that).
static int host_copy_threads() {
    static const int n = [] {
        int c = 0;
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) c = CPU_COUNT(&set);
        if (c <= 0) c = (int)std::thread::hardware_concurrency();
        if (FILE* f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
            char q[32] = {0}; long per = 0;
            if (fscanf(f, "%31s %ld", q, &per) == 2 && strcmp(q, "max") != 0 && per > 0) {
                const long quota = atol(q);
                if (quota > 0) c = std::min(c, std::max(1, (int)((quota + per / 2) / per)));
            }
            fclose(f);
        }
        if (getenv("GITCAP_HOST_COPY_THREADS")) c = atoi(getenv("GITCAP_HOST_COPY_THREADS"));
        return std::max(1, std::min(8, c));
    }();
    return n;
}

int gitcap_host_copy(void* dst, const void* src, int64_t bytes) {
    if ((!dst || !src) && bytes > 0) return GITCAP_ERR_ARG;
    if (bytes <= 0) return bytes == 0 ? 0 : GITCAP_ERR_ARG;
    const int64_t piece = (int64_t)4 << 20;                        // below 4 MiB per thread a second thread does not pay
    int nt = (int)std::min<int64_t>(host_copy_threads(), (bytes + piece - 1) / piece);
    if (nt <= 1) { memcpy(dst, src, (size_t)bytes); return 0; }
    const int64_t chunk = ((bytes + nt - 1) / nt + 4095) & ~(int64_t)4095;
    std::vector<std::thread> th;
    th.reserve(nt - 1);
    int started = 0;
    try {
        for (int i = 1; i < nt; ++i) {
            const int64_t o = chunk * i;
            if (o >= bytes) break;
            th.emplace_back([=] { memcpy((char*)dst + o, (const char*)src + o, (size_t)std::min(chunk, bytes - o)); });
            ++started;
        }
    } catch (...) {                                                 // no thread to be had: the caller's thread copies the rest
        for (auto& t : th) t.join();
        const int64_t o = chunk * (started + 1);
        memcpy(dst, src, (size_t)std::min(chunk, bytes));
        if (o < bytes) memcpy((char*)dst + o, (const char*)src + o, (size_t)(bytes - o));
        return 0;
    }
    memcpy(dst, src, (size_t)std::min(chunk, bytes));
    for (auto& t : th) t.join();
    return 0;
}

int gitcap_dbg_enc_tap(gitcap_t* h, float* buf) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "dbg_enc_tap: null handle");
    h->enc_tap = buf;
    return 0;
}

int gitcap_hidden_states_enable(gitcap_t* h, int enable) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "hidden_states_enable: null handle");
    GUARD(h);
    select_slot(h, 0);
    if (enable && !h->hid_img) {
        const size_t n = (size_t)h->c.dec_layers + 1;
        int rc = dev_alloc(h, &h->hid_img, n * h->Mi * h->D);
        rc = rc ? rc : dev_alloc(h, &h->hid_txt, n * h->Mt * h->D);
        if (rc) return rc;
    }
    h->want_hidden = enable != 0;
    cur(h).have = false;     // the image rows of the last layer are only computed while this is on
    return 0;
}

int gitcap_hidden_states_read(gitcap_t* h, int B, int S_img, int T, float* out, void* stream) {
    if (!h || !out) return fail(h, GITCAP_ERR_ARG, "hidden_states_read: null argument");
    GUARD(h);
    select_slot(h, 0);
    const gitcap::Slot& sl = cur(h);
    if (!h->want_hidden || !sl.have) return fail(h, GITCAP_ERR_STATE, "hidden_states_read: enable, encode and run a prefix (t0 = 0) first");
    if (sl.ragged) return fail(h, GITCAP_ERR_ARG, "hidden_states_read: the image prefix is a ragged batch (gitcap_attach_frame_counts), whose rows have no [B][S_img] layout");
    if (B != sl.B || S_img != sl.S || T != h->hid_T || T <= 0)
        return fail(h, GITCAP_ERR_ARG, "hidden_states_read: B / S_img / T differ from the last encode + text_forward");
    HIP_OK(h, launch_gather_hidden(h->hid_img, h->hid_txt, out, h->c.dec_layers + 1, B, S_img, T, h->D, (size_t)h->Mi * h->D,
                                   (size_t)h->Mt * h->D, (hipStream_t)stream));
    return 0;
}

int gitcap_set_weight_storage(gitcap_t* h, int storage) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "set_weight_storage: null handle");
    if (storage != GITCAP_W_BF16 && storage != GITCAP_W_FP8_E4M3) return fail(h, GITCAP_ERR_ARG, "set_weight_storage: unknown storage");
    for (auto& kv : h->w)
        if (kv.second.loaded && kv.second.kind == 1) return fail(h, GITCAP_ERR_STATE, "set_weight_storage: call it before the first gitcap_load_tensor");
    h->fp8 = storage == GITCAP_W_FP8_E4M3;
    return 0;
}

int gitcap_set_kv_cache(gitcap_t* h, int mode) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "set_kv_cache: null handle");
    if (mode != GITCAP_KV_BF16 && mode != GITCAP_KV_V_E4M3) return fail(h, GITCAP_ERR_ARG, "set_kv_cache: unknown mode");
    GUARD(h);
    HIP_OK(h, hipDeviceSynchronize());          // not between the launches of a submission in flight
    select_slot(h, 0);
    if (mode == GITCAP_KV_V_E4M3 && !h->slots[0].v8_img) {
        for (auto& sl : h->slots) {
            int rc = dev_alloc(h, &sl.v8_img, (size_t)h->c.dec_layers * h->Mi * h->D);
            rc = rc ? rc : dev_alloc(h, &sl.vs_img, (size_t)h->c.dec_layers * h->Mi * h->c.dec_heads);
            if (rc) return rc;
        }
    }
    h->kv_v8 = mode == GITCAP_KV_V_E4M3;
    for (auto& sl : h->slots) sl.have = false;
    return 0;
}

int gitcap_set_compute(gitcap_t* h, int compute) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "set_compute: null handle");
    if (compute != GITCAP_COMPUTE_BF16 && compute != GITCAP_COMPUTE_FP8_FFN) return fail(h, GITCAP_ERR_ARG, "set_compute: unknown mode");
    GUARD(h);
    if (compute == GITCAP_COMPUTE_FP8_FFN) {
        const gitcap_config& c = h->c;
        if (!h->fp8) return fail(h, GITCAP_ERR_STATE, "set_compute(fp8_ffn): needs e4m3 weight storage (gitcap_set_weight_storage first)");
        auto ok_ln = [](int n) { return n == 768 || n == 1024; };
        if (!ok_ln(c.enc_width) || !ok_ln(c.dec_width) || c.enc_ffn % 256 || c.dec_ffn % 256)
            return fail(h, GITCAP_ERR_ARG, "set_compute(fp8_ffn): widths must be 768 or 1024 and the FFN widths multiples of 256");
        if (!h->hb8) {
            const size_t Dm = std::max(h->Dv, h->D), Fm = std::max(c.enc_ffn, c.dec_ffn);
            int rc = dev_alloc(h, &h->hb8, (size_t)h->Mi * Dm);
            rc = rc ? rc : dev_alloc(h, &h->ffn8, (size_t)h->Mi * Fm);
            rc = rc ? rc : dev_alloc(h, &h->f8_sat, 1);
            if (rc) return rc;
        }
    }
    HIP_OK(h, hipDeviceSynchronize());          // not between the launches of a submission in flight
    h->f8ffn = compute == GITCAP_COMPUTE_FP8_FFN;
    cur(h).have = false;
    return 0;
}

int gitcap_set_fp8_scale(gitcap_t* h, float scale) {
    if (!h) return fail(h, GITCAP_ERR_ARG, "set_fp8_scale: null handle");
    int e = 0;
    if (!(scale > 0.f) || std::frexp(scale, &e) != 0.5f || e < -15 || e > 9)          // 2^-16 .. 2^8
        return fail(h, GITCAP_ERR_ARG, "set_fp8_scale: the scale must be a power of two in [2^-16, 2^8]");
    GUARD(h);
    HIP_OK(h, hipDeviceSynchronize());          // not between the launches of a submission in flight
    h->f8_scale = scale;
    cur(h).have = false;
    return 0;
}

int gitcap_fp8_saturations(gitcap_t* h, int64_t* count, int reset) {
    if (!h || !count) return fail(h, GITCAP_ERR_ARG, "fp8_saturations: null argument");
    GUARD(h);
    *count = 0;
    if (!h->f8_sat) return 0;                   // compute = fp8_ffn was never selected: nothing was ever encoded
    HIP_OK(h, hipDeviceSynchronize());
    unsigned long long v = 0;
    HIP_OK(h, hipMemcpy(&v, h->f8_sat, sizeof(v), hipMemcpyDeviceToHost));
    if (reset) HIP_OK(h, hipMemset(h->f8_sat, 0, sizeof(v)));
    *count = (int64_t)v;
    return 0;
}

int gitcap_weight_bytes(const gitcap_t* h, int64_t* bytes) {
    if (!h || !bytes) return GITCAP_ERR_ARG;
    *bytes = h->weight_bytes;
    return 0;
}

int gitcap_workspace_bytes(const gitcap_t* h, int64_t* bytes) {
    if (!h || !bytes) return GITCAP_ERR_ARG;
    *bytes = h->ws_bytes + h->win_bytes + h->pool_bytes;
    return 0;
}

}  // extern "C"
