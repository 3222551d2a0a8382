// Host-only logic of libgitcap, free of any HIP dependency so that it also compiles for the CPU under
// -fsanitize=address,undefined (`make asan`, tests/test_host_asan.py): numeric encodings of the weight loader, the
// canonical tensor table, the pipeline's ticket -> slot bookkeeping, the window rings' cursor, the stream pool's slot plan
// (`make asan-pool`, host_pool_asan_test.cpp) and the workgroup -> tile map of the residual +
// LayerNorm GEMM (shared with the kernel, which compiles the same function for the device).
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/gitcap.h"

#if defined(__HIPCC__)
#define GITCAP_HD __host__ __device__
#else
#define GITCAP_HD
#endif

inline int pad_to(int v, int m) { return (v + m - 1) / m * m; }

// an on/off environment switch: set and neither empty nor "0"
inline bool env_flag(const char* name) {
    const char* v = getenv(name);
    return v && v[0] && !(v[0] == '0' && v[1] == 0);
}

inline uint16_t host_f2bf(float f) {    // round-to-nearest-even, NaN stays NaN
    uint32_t u;
    memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u) return (uint16_t)((u >> 16) | 0x40);
    u += 0x7fffu + ((u >> 16) & 1u);
    return (uint16_t)(u >> 16);
}

// OCP e4m3fn code of x, or -1 when x is not exactly representable (bias 7, 3 mantissa bits, max 448, no infinities)
inline int host_e4m3_exact(float x) {
    const int sign = std::signbit(x) ? 0x80 : 0;
    const float a = std::fabs(x);
    if (a == 0.f) return sign;
    if (!(a <= 448.f)) return -1;
    int e;
    const float m = std::frexp(a, &e);          // a = m * 2^e, m in [0.5, 1)
    const int E = e - 1 + 7;                    // a = (2m) * 2^(e-1)
    if (E >= 1) {
        const float f = (2.f * m - 1.f) * 8.f;  // mantissa field
        const int M = (int)f;
        if ((float)M != f) return -1;
        return sign | (E << 3) | M;
    }
    const float f = std::ldexp(a, 9);           // subnormal: a = M * 2^-9
    const int M = (int)f;
    if ((float)M != f || M < 1 || M > 7) return -1;
    return sign | M;
}

// value of an e4m3fn code (0x7f / 0xff are NaN)
inline float host_e4m3_value(int code) {
    const int E = (code >> 3) & 15, M = code & 7;
    if (E == 15 && M == 7) return NAN;
    const float a = E ? std::ldexp(1.f + M / 8.f, E - 7) : std::ldexp((float)M, -9);
    return (code & 0x80) ? -a : a;
}

// the power-of-two row scale of e4m3 storage: the smallest 2^e with amax / 2^e <= 448
inline float host_e4m3_row_scale(const float* row, int64_t cols) {
    float amax = 0.f;
    for (int64_t k = 0; k < cols; ++k) amax = std::fmax(amax, std::fabs(row[k]));
    int e = 0;
    if (amax > 0.f) { (void)std::frexp(amax / 448.0f, &e); if (std::ldexp(1.0f, e - 1) * 448.0f >= amax) --e; }
    return std::ldexp(1.0f, e);
}

// Encodes one row (cols values -> q[0..cols), the caller zero-pads up to its row pitch); false when a value is not
// e4m3 x scale exactly (the loader refuses instead of rounding).
inline bool host_e4m3_encode_row(const float* row, int64_t cols, float scale, uint8_t* q) {
    for (int64_t k = 0; k < cols; ++k) {
        const int code = host_e4m3_exact(row[k] / scale);
        if (code < 0) return false;
        q[k] = (uint8_t)code;
    }
    return true;
}

// canonical names -> shape; mirrors gitcap/weights.py:canonical_shapes
inline void expected_shapes(const gitcap_config& c, std::vector<std::pair<std::string, std::vector<int64_t>>>& out) {
    const int64_t Dv = c.enc_width, D = c.dec_width, V = c.vocab_size;
    const int64_t G = c.image_size / c.patch_size, N = G * G + 1, pd = 3LL * c.patch_size * c.patch_size;
    auto add = [&](const std::string& n, std::vector<int64_t> s) { out.emplace_back(n, std::move(s)); };
    add("enc.patch_w", {Dv, pd}); add("enc.cls", {Dv}); add("enc.pos", {N, Dv});
    add("enc.ln_pre.w", {Dv}); add("enc.ln_pre.b", {Dv}); add("enc.ln_post.w", {Dv}); add("enc.ln_post.b", {Dv});
    for (int i = 0; i < c.enc_layers; ++i) {
        const std::string p = "enc.L" + std::to_string(i) + ".";
        add(p + "ln1.w", {Dv}); add(p + "ln1.b", {Dv});
        add(p + "qkv.w", {3 * Dv, Dv}); add(p + "qkv.b", {3 * Dv});
        add(p + "proj.w", {Dv, Dv}); add(p + "proj.b", {Dv});
        add(p + "ln2.w", {Dv}); add(p + "ln2.b", {Dv});
        add(p + "fc1.w", {c.enc_ffn, Dv}); add(p + "fc1.b", {c.enc_ffn});
        add(p + "fc2.w", {Dv, c.enc_ffn}); add(p + "fc2.b", {Dv});
    }
    add("temporal", {c.num_frames > 1 ? c.num_frames : 1, Dv});
    add("vproj.w", {D, Dv}); add("vproj.b", {D}); add("vproj.ln.w", {D}); add("vproj.ln.b", {D});
    add("txt.word", {V, D}); add("txt.pos", {c.max_text_pos, D}); add("txt.ln.w", {D}); add("txt.ln.b", {D});
    for (int i = 0; i < c.dec_layers; ++i) {
        const std::string p = "dec.L" + std::to_string(i) + ".";
        add(p + "qkv.w", {3 * D, D}); add(p + "qkv.b", {3 * D});
        add(p + "ao.w", {D, D}); add(p + "ao.b", {D});
        add(p + "ln1.w", {D}); add(p + "ln1.b", {D});
        add(p + "fc1.w", {c.dec_ffn, D}); add(p + "fc1.b", {c.dec_ffn});
        add(p + "fc2.w", {D, c.dec_ffn}); add(p + "fc2.b", {D});
        add(p + "ln2.w", {D}); add(p + "ln2.b", {D});
    }
    add("head.w", {V, D}); add("head.b", {V});
}

inline bool is_gemm_weight(const std::string& n) {
    if (n == "enc.patch_w" || n == "vproj.w" || n == "head.w") return true;
    auto ends = [&](const char* s) { size_t l = strlen(s); return n.size() >= l && n.compare(n.size() - l, l, s) == 0; };
    return ends("qkv.w") || ends("proj.w") || ends("fc1.w") || ends("fc2.w") || ends("ao.w");
}

// One entry of a handle's weight table (GIT, student, TinyViT): what *_load_tensor expects and what it uploaded.
struct DevTensor {
    void* p = nullptr;
    std::vector<int64_t> shape;   // logical (unpadded) shape
    int kind = 0;                 // 0 fp32 as loaded, 1 GEMM weight (bf16 panel, or e4m3 + row scales), 2 depthwise [9][C] (TinyViT)
    bool loaded = false;
    int64_t bytes = 0;            // device bytes held (incl. row scales)
};
// The shared head of the three *_load_tensor entry points: the table's entry for `name` once rank and shape agree with it,
// else nullptr and the message in `err`, led by the caller's prefix ("load_tensor", "student_load_tensor", ...).
inline DevTensor* find_tensor(std::map<std::string, DevTensor>& table, const char* name, const int64_t* shape, int rank,
                              const char* prefix, std::string& err) {
    auto it = table.find(name);
    if (it == table.end()) { err = std::string(prefix) + ": unknown tensor '" + name + "'"; return nullptr; }
    DevTensor& t = it->second;
    if ((int)t.shape.size() != rank) { err = std::string(prefix) + ": rank mismatch for " + name; return nullptr; }
    for (int i = 0; i < rank; ++i)
        if (t.shape[i] != shape[i]) { err = std::string(prefix) + ": shape mismatch for " + name; return nullptr; }
    return &t;
}

// Pipeline bookkeeping (gitcap_greedy_submit / _wait): submission t uses slot t % nslot; a ticket can be waited for
// while its slot has not been handed to a later submission.
inline int ticket_slot(int ticket, int nslot) { return ticket % nslot; }
inline bool ticket_waitable(int ticket, int next_ticket, int nslot) {
    return ticket >= 0 && ticket < next_ticket && ticket >= next_ticket - nslot;
}
// A failed statistics exchange (ExchangeHealth below) leaves every submission made so far with undefined results: the handle keeps
// the ticket count at that moment (`poison_upto`), and a wait on a ticket below it is refused every time it is asked for, so a retry
// cannot hand the ids out (gitcap_greedy_wait / gitcap_beam_search_wait).  Tickets submitted afterwards run on the unfused launches.
inline int poison_mark(int next_ticket) { return next_ticket; }
inline bool ticket_poisoned(int ticket, int poison_upto) { return ticket < poison_upto; }

// Window ring (the teacher's frame window and the student's memory-token window): `slots` entries per clip, head = the slot the
// next entry goes to (the oldest entry once the ring is full), count = entries pushed since the reset, capped at slots.
struct RingCursor {
    int slots = 0, head = 0, count = 0;
    void reset(int n) { slots = n; head = count = 0; }
    int first_run(int n) const { return n < slots - head ? n : slots - head; }      // of n <= slots new entries, those up to the wrap
    void push(int n) { head = (head + n) % slots; count = count + n < slots ? count + n : slots; }
    bool full() const { return slots > 0 && count >= slots; }
    void clear() { count = 0; }     // the entries may be undefined (a failed push, a failed exchange): pushed again by the caller
    int oldest() const { return (head + slots - count) % slots; }      // slot of the oldest entry held (count <= slots; 1 <= count)
};

// Stream pool (gitcap_student_pool_*): S independent rings in one buffer, one RingCursor per stream; ring row = stream * slots + slot.
// One push holds tokens for any streams in any mix: token i goes to stream ids[i] behind that stream's earlier tokens, this
// push's earlier ones included.  pool_push_slots writes slot[i] = the ring row of token i and changes nothing; a stream may get at
// most `slots` tokens per push (more would write one row twice in one launch).  *bad = the first token refused.
enum { POOL_PUSH_OK = 0, POOL_PUSH_BAD_ID = 1, POOL_PUSH_OVER = 2 };
inline int pool_push_slots(const std::vector<RingCursor>& cur, const int32_t* ids, int n, int32_t* slot, int* bad) {
    std::vector<int> seen(cur.size(), 0);
    for (int i = 0; i < n; ++i) {
        const int32_t id = ids[i];
        *bad = i;
        if (id < 0 || (size_t)id >= cur.size()) return POOL_PUSH_BAD_ID;
        const RingCursor& c = cur[(size_t)id];
        const int j = seen[(size_t)id]++;
        if (j >= c.slots) return POOL_PUSH_OVER;
        slot[i] = id * c.slots + (c.head + j) % c.slots;
    }
    *bad = -1;
    return POOL_PUSH_OK;
}
// the cursors behind a push that pool_push_slots accepted
inline void pool_push_commit(std::vector<RingCursor>& cur, const int32_t* ids, int n) {
    for (int i = 0; i < n; ++i) cur[(size_t)ids[i]].push(1);
}

// The teacher's stream pool (gitcap_pool_*): the ring holds FRAMES (ring frame = stream * slots + slot), and one plan maps the
// cursors to every table a push and a pool call need.  First the push: frame i of `push_ids` [n_push] goes to ring frame dst[i]
// (pool_push_slots' rule) and the cursors advance.  Then the call on the cursors behind that push: decoder row r = stream
// cap_ids[r], its last len[r] = count frames, oldest first, packed behind row r - 1's from packed frame off[r] on; packed frame g
// is ring frame src[g] and the pos[g]-th frame of its own clip (the temporal embedding it gets).  total = packed frames, maxn =
// the longest row's, dense = every row holds the same number (the packed layout is then [B][n] and the call takes the dense
// launches).  n_push == 0 / B == 0 leave that half out.  A refused plan changes nothing: *bad = the push frame or the row refused.
enum { POOL_PLAN_OK = 0, POOL_PLAN_BAD_ID = 1, POOL_PLAN_OVER = 2, POOL_PLAN_TWICE = 3, POOL_PLAN_EMPTY = 4 };
struct PoolPlan { int total = 0, maxn = 0; bool dense = true; };
inline int pool_plan(std::vector<RingCursor>& cur, const int32_t* push_ids, int n_push, int32_t* dst, const int32_t* cap_ids, int B,
                     int32_t* src, int32_t* pos, int32_t* off, int32_t* len, PoolPlan* plan, int* bad) {
    *plan = PoolPlan{};
    if (n_push > 0)
        if (const int why = pool_push_slots(cur, push_ids, n_push, dst, bad)) return why;      // (the two enums agree on 0, 1, 2)
    std::vector<RingCursor> after = cur;
    if (n_push > 0) pool_push_commit(after, push_ids, n_push);
    for (int r = 0; r < B; ++r) {
        const int32_t id = cap_ids[r];
        *bad = r;
        if (id < 0 || (size_t)id >= after.size()) return POOL_PLAN_BAD_ID;
        for (int q = 0; q < r; ++q)
            if (cap_ids[q] == id) return POOL_PLAN_TWICE;
        if (after[(size_t)id].count < 1) return POOL_PLAN_EMPTY;
    }
    int g = 0;
    for (int r = 0; r < B; ++r) {
        const RingCursor& c = after[(size_t)cap_ids[r]];
        off[r] = g; len[r] = c.count;
        for (int f = 0; f < c.count; ++f, ++g) { src[g] = cap_ids[r] * c.slots + (c.oldest() + f) % c.slots; pos[g] = f; }
        plan->maxn = c.count > plan->maxn ? c.count : plan->maxn;
        plan->dense = plan->dense && c.count == len[0];
    }
    plan->total = g;
    cur.swap(after);
    *bad = -1;
    return POOL_PLAN_OK;
}

// ---- per-call options: the one-shot attachments of gitcap_attach_* --------------------------------------------------------
// Each setter writes its part of the handle's `pending` record; an entry point states which parts it takes and which it refuses,
// and the taken parts are the handle's `call` record -- the options of the call whose launches are being issued -- until it returns.
// token log-probabilities (*_attach_token_logprobs): device fp32 [B][ld]; p == nullptr: none
struct LpAttach { float* p = nullptr; int ld = 0; };
// A batch of prompts (gitcap_attach_prompt): ids device int64 [rows][ld], lengths device int32 [rows] = valid tokens per row (the
// kernels clamp them to [1, max_len]; max_len <= ld, so a wrong length reads no other row), min_len / max_len = the host's bounds.
// ids == nullptr: none.  (Travels to the kernels by value, as RaggedCounts: plain members only.)
struct PromptArgs { const int64_t* ids; int ld; const int32_t* lengths; int min_len, max_len; };
// Ragged batches (gitcap_attach_frame_counts): clips of 1..255 frames each, packed clip-major; B == 0: none
struct RaggedCounts { int B; unsigned char n[256]; };
// Options of one device-resident search (gitcap_attach_search_options): hypotheses kept per clip, repetition penalty, n-best outputs
// (n = 1, rp = 1: none).  smp: the sampling branch (gitcap_attach_sampling), pending beside the options above and consumed with them.
struct SampleOpt { bool on = false; float temperature = 1.0f; int top_k = 0; float top_p = 1.0f; uint64_t seed = 0; };
struct SearchOpt { int n = 1; float rp = 1.0f; int64_t* nbest = nullptr; float* nbest_lp = nullptr; SampleOpt smp{}; };
// gitcap_attach_constraints: what a step may not emit (include/gitcap.h); on = false: none
struct ConsOpt { bool on = false; int ngram = 0, min_length = 0; const int32_t* suppress = nullptr; int n_suppress = 0; };

// top-k alternatives per position (*_attach_top_logprobs): device int64 / fp32 [B][ld][k]; k == 0: none
struct TopkAttach { int k = 0; int64_t* ids = nullptr; float* lp = nullptr; int ld = 0; };

struct CallOpts { LpAttach lp{}; SearchOpt so{}; PromptArgs pr{}; ConsOpt co{}; RaggedCounts fc{}; TopkAttach tk{}; };
enum : unsigned { OPT_LP = 1, OPT_SO = 2, OPT_PR = 4, OPT_CO = 8, OPT_FC = 16, OPT_TK = 32 };

inline unsigned opts_set(const CallOpts& o) {       // the parts that hold an attachment
    return (o.lp.p ? OPT_LP : 0u) | (o.so.n != 1 || o.so.rp != 1.0f || o.so.smp.on ? OPT_SO : 0u) | (o.pr.ids ? OPT_PR : 0u) |
           (o.co.on ? OPT_CO : 0u) | (o.fc.B != 0 ? OPT_FC : 0u) | (o.tk.k != 0 ? OPT_TK : 0u);
}
inline void opts_clear(CallOpts& o, unsigned parts) {
    if (parts & OPT_LP) o.lp = LpAttach{};
    if (parts & OPT_SO) o.so = SearchOpt{};
    if (parts & OPT_PR) o.pr = PromptArgs{};
    if (parts & OPT_CO) o.co = ConsOpt{};
    if (parts & OPT_FC) o.fc.B = 0;
    if (parts & OPT_TK) o.tk = TopkAttach{};
}
// The student's record (gitcap_student_attach_*): the same parts with search options of its own, and counts that are a vector -- its
// max_rows may exceed the 256 clips RaggedCounts holds (empty: none; an empty vector is copied without an allocation).
// se (gitcap_student_attach_search, part OPT_SO): the beam family's search that ends hypotheses at SEP -- n hypotheses kept per clip,
// the length penalty, pn candidates per beam (resolved: 0 never gets here), the repetition penalty, and where the n scores and
// lengths per clip go (device [B][n]; lengths nullable).  on = false: none.
struct StudentSearch { bool on = false; int n = 1; float length_penalty = 1.0f; int pn = 0; float rp = 1.0f; float* scores = nullptr; int32_t* lengths = nullptr; };
struct StudentOpts { LpAttach lp{}; TopkAttach tk{}; ConsOpt co{}; PromptArgs pr{}; std::vector<int32_t> fc; StudentSearch se{}; };
inline unsigned opts_set(const StudentOpts& o) {
    return (o.lp.p ? OPT_LP : 0u) | (o.pr.ids ? OPT_PR : 0u) | (o.co.on ? OPT_CO : 0u) | (!o.fc.empty() ? OPT_FC : 0u) | (o.tk.k != 0 ? OPT_TK : 0u) |
           (o.se.on ? OPT_SO : 0u);
}
inline void opts_clear(StudentOpts& o, unsigned parts) {
    if (parts & OPT_SO) o.se = StudentSearch{};
    if (parts & OPT_LP) o.lp = LpAttach{};
    if (parts & OPT_PR) o.pr = PromptArgs{};
    if (parts & OPT_CO) o.co = ConsOpt{};
    if (parts & OPT_FC) o.fc.clear();
    if (parts & OPT_TK) o.tk = TopkAttach{};
}
// The parts in `take` move out of `pending` into the result (consumed, whatever becomes of the call); the parts in `refuse` are
// cleared, *refused = those of them that held an attachment; every other part stays pending.  (CallOpts or StudentOpts.)
template <class Opts>
Opts take_opts(Opts& pending, unsigned take, unsigned refuse, unsigned* refused) {
    *refused = opts_set(pending) & refuse;
    Opts out = pending;
    opts_clear(out, ~take);
    opts_clear(pending, take | refuse);
    return out;
}
// An entry point's take: `call` holds the taken parts while the scope lives and is empty again on every exit.
struct CallScope {
    CallOpts& call;
    unsigned refused = 0;
    CallScope(CallOpts& pending, CallOpts& call_, unsigned take, unsigned refuse) : call(call_) { call = take_opts(pending, take, refuse, &refused); }
    ~CallScope() { call = CallOpts{}; }
    CallScope(const CallScope&) = delete;
    CallScope& operator=(const CallScope&) = delete;
};
// the message of a call that refuses an attachment: frame counts (the default: what most refusals are about), or the top-k
// alternatives a draft call does not carry; names the attachment and its setter
inline std::string refused_message(const char* who, unsigned part = OPT_FC) {
    if (part & OPT_TK)
        return std::string(who) + ": top-k alternatives are attached (gitcap_attach_top_logprobs), which this call does not take";
    return std::string(who) + ": per-clip frame counts are attached (gitcap_attach_frame_counts), which this call does not take";
}

// ---- the tail of a draft verified row by row (gitcap_greedy_draft) ---------------------------------------------------------
// The accept launch reports min / max over the captions of covered_r (the steps the verify pass settled for caption r) and whether
// all rows emitted SEP in one of the steps every caption covers.  The token loop goes on at the first step some caption lacks,
// t_first = min covered -- captions ahead of it recompute K/V from the tokens they already hold, the same bits -- unless nothing is
// left (t_first >= max_len) or the stop rule (stop_all_sep) has fired.  keep_below: step t writes position t + 1, which a caption
// holds already while t + 1 < 1 + covered_r: steps with t + 1 < keep_below = 1 + max covered run the KEEP arg-max, the rest the plain one.
struct DraftTail { bool run; int t_first, keep_below, steps; };
inline DraftTail draft_tail_plan(int min_covered, int max_covered, bool fired, int max_len, bool stop_all_sep) {
    DraftTail p{};
    p.t_first = min_covered;
    p.keep_below = 1 + max_covered;
    p.run = min_covered < max_len && !(stop_all_sep && fired);
    p.steps = p.run ? max_len - min_covered : 0;
    return p;
}
inline bool draft_keep_step(const DraftTail& p, int t) { return t + 1 < p.keep_below; }

// ---- residual + LayerNorm GEMM: workgroup -> tile ----------------------------------------------------------------
// The N/256 tiles of a 256-row block wait for each other (statistics exchange, gemm_epilogue.h), so they must be
// consecutive workgroups of ONE XCD's dispatch sequence.  Workgroup b runs on XCD b % 8 as that XCD's (b / 8)-th
// workgroup: XCD x is handed a balanced contiguous range of WHOLE row blocks, their ntn tiles consecutive in its
// sequence.  The grid is padded to 8 * ntn * ceil(nrb / 8); surplus workgroups (the last of every sequence) get no tile.
GITCAP_HD inline int ln_grid_size(int nrb, int ntn) { return 8 * ntn * ((nrb + 7) >> 3); }
// When to use that map: only where it is needed for progress, i.e. on grids of more than 256 tiles, which run in several
// rounds.  A grid that fits the chip is co-resident whatever the map and keeps the plain XCD remap, whose even spread
// (222 tiles: 28 / 27 per XCD) leaves every XCD free CUs for the token-loop kernels of the other streams: handing XCDs
// whole row blocks there (30 / 27) cost the pipelined bench 5 % (1651 vs 1742 captions/s, same box, round 3).
// `cus` = compute units of the device the launch goes to (hipDeviceProp_t::multiProcessorCount, device_cus() in kernels.h:
// 256 on a whole MI355X, fewer on a partitioned one).
inline bool ln_use_rowblock_map(int nrb, int ntn, int cus = 256) { return nrb * ntn > cus; }
GITCAP_HD inline bool ln_tile_of_block(int bid, int nrb, int ntn, int* tm, int* tn) {
    const int xcd = bid & 7, slot = bid >> 3;
    const int c = nrb >> 3, r = nrb & 7;
    const int cnt = c + (xcd < r ? 1 : 0), start = xcd * c + (xcd < r ? xcd : r);
    const int j = slot / ntn;
    if (j >= cnt) return false;
    *tm = start + j; *tn = slot - j * ntn;
    return true;
}

// ---- health of the GEMM + LayerNorm statistics exchange -------------------------------------------------------------------
// A tile of a fused launch waits (bounded) for the sibling tiles of its row block; if the bound is ever hit -- the siblings
// cannot become resident, e.g. a foreign process or a CU-masked stream holds the CUs (co-residency) -- the
// kernel does not trap: it raises a word in host-visible memory and finishes with undefined LayerNorm output.  The host
// reads the word at every entry point (and in gitcap_poll_errors): once raised, the launches issued since the last clean
// check are suspect, the handle switches for good to GEMM + row-kernel launches (same bits, no exchange) and the entry
// point returns GITCAP_ERR_EXCHANGE so that the caller re-runs what it had in flight.
struct ExchangeHealth {
    bool degraded = false;      // fused epilogues switched off for this handle
    int trips = 0;              // times the flag was found raised
};
// flag = the value read from the host-visible word.  Returns true when the caller must reset (sync, clear the word and the
// exchange barriers) and report GITCAP_ERR_EXCHANGE.
inline bool exchange_poll(ExchangeHealth& hs, unsigned flag) {
    if (!flag) return false;
    hs.degraded = true;
    ++hs.trips;
    return true;
}
