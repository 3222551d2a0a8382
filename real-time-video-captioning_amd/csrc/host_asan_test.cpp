// CPU-only driver of the host logic under AddressSanitizer + UBSan (`make asan`): no HIP, no GPU.
#include "host_logic.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "host_asan_test: %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// Per-call options: what each family of entry points takes and refuses (the masks gitcap.hip states), on a record with every part
// attached.  `early`: the call returns before its body, as one refused for its arguments does.
static CallOpts all_attached(float* lp, int64_t* nb, const int64_t* ids, const int32_t* len) {
    CallOpts o{};
    o.lp = LpAttach{lp, 8};
    o.so = SearchOpt{2, 1.5f, nb, lp, SampleOpt{true, 0.7f, 5, 1.0f, 9}};
    o.pr = PromptArgs{ids, 4, len, 1, 3};
    o.co = ConsOpt{true, 2, 3, len, 1};
    o.fc.B = 3; o.fc.n[0] = 2; o.fc.n[1] = 255; o.fc.n[2] = 1;
    return o;
}
static int entered(CallOpts& pending, CallOpts& call, unsigned take, unsigned refuse, bool early, unsigned* seen, unsigned* refused) {
    CallScope scope(pending, call, take, refuse);
    *seen = opts_set(call);
    *refused = scope.refused;
    if (early) return 1;
    CHECK(&scope.call == &call);
    return 0;
}
static int call_opts_test() {
    float lp[1]; int64_t nb[1]; const int64_t ids[1] = {0}; const int32_t len[1] = {1};
    const unsigned ALL = OPT_LP | OPT_SO | OPT_PR | OPT_CO | OPT_FC, GREEDY = OPT_LP | OPT_PR | OPT_CO, BEAM = OPT_SO | OPT_PR | OPT_CO;
    { CallOpts none{}; CHECK(opts_set(none) == 0 && opts_set(all_attached(lp, nb, ids, len)) == ALL); }
    struct Row { unsigned take, refuse; } rows[] = {
        {GREEDY | OPT_FC, 0},       // gitcap_greedy, _raw, _submit, _raw_submit
        {GREEDY, OPT_FC},           // gitcap_window_greedy
        {BEAM | OPT_FC, 0},         // gitcap_beam_search, _submit, _raw_submit
        {BEAM, OPT_FC},             // gitcap_window_beam_search
        {OPT_FC, 0},                // gitcap_encode, gitcap_encode_raw
        {0, OPT_FC},                // gitcap_set_visual, gitcap_window_reset, gitcap_window_push(_raw)
        {0, 0},                     // score, distill, text_forward: everything stays pending
    };
    for (const Row& r : rows)
        for (int early = 0; early < 2; ++early) {
            CallOpts pending = all_attached(lp, nb, ids, len), call{};
            unsigned seen = 0, refused = 0;
            CHECK(entered(pending, call, r.take, r.refuse, early != 0, &seen, &refused) == early);
            CHECK(seen == r.take && refused == r.refuse);                     // the body sees exactly the taken parts
            CHECK(opts_set(call) == 0 && call.fc.B == 0);                     // the scope emptied `call`, on the early return too
            CHECK(opts_set(pending) == (ALL & ~(r.take | r.refuse)));         // taken (even by a failed call) and refused: gone
            // a second call finds nothing to take or refuse, and what stayed pending is intact
            CHECK(entered(pending, call, r.take, r.refuse, false, &seen, &refused) == 0 && seen == 0 && refused == 0);
            if (!(r.take & OPT_LP)) CHECK(pending.lp.p == lp && pending.lp.ld == 8);
            if (!(r.take & OPT_SO)) CHECK(pending.so.n == 2 && pending.so.rp == 1.5f && pending.so.nbest == nb && pending.so.smp.on && pending.so.smp.seed == 9);
            if (!(r.take & OPT_PR)) CHECK(pending.pr.ids == ids && pending.pr.lengths == len && pending.pr.max_len == 3);
            if (!(r.take & OPT_CO)) CHECK(pending.co.on && pending.co.ngram == 2 && pending.co.n_suppress == 1);
            if (!((r.take | r.refuse) & OPT_FC)) CHECK(pending.fc.B == 3 && pending.fc.n[1] == 255);
        }
    // the taken values arrive whole; nothing is refused where nothing is attached; sampling alone counts as search options
    {
        CallOpts pending = all_attached(lp, nb, ids, len);
        unsigned refused = 7;
        const CallOpts got = take_opts(pending, BEAM | OPT_FC, 0, &refused);
        CHECK(refused == 0 && got.lp.p == nullptr && got.so.n == 2 && got.so.nbest_lp == lp && got.so.smp.top_k == 5 && got.pr.min_len == 1);
        CHECK(got.co.suppress == len && got.fc.B == 3 && got.fc.n[0] == 2 && got.fc.n[2] == 1 && pending.lp.p == lp);
        CHECK(pending.so.n == 1 && pending.so.rp == 1.0f && !pending.so.smp.on && !pending.pr.ids && !pending.co.on && pending.fc.B == 0);
        (void)take_opts(pending, 0, OPT_FC, &refused);
        CHECK(refused == 0);
        CallOpts smp{};
        smp.so.smp.on = true;
        CHECK(opts_set(smp) == OPT_SO);
    }
    CHECK(refused_message("window") == "window: per-clip frame counts are attached (gitcap_attach_frame_counts), which this call does not take");
    return 0;
}

// top-k alternatives (OPT_TK): a part like the others -- taken by the greedy family and score, refused (and consumed) by a draft
// call, left pending by the beam family
static int topk_opts_test() {
    float lp[1]; int64_t nb[1]; const int64_t ids[1] = {0}; const int32_t len[1] = {1};
    const unsigned ALL = OPT_LP | OPT_SO | OPT_PR | OPT_CO | OPT_FC, GREEDY = OPT_LP | OPT_PR | OPT_CO, BEAM = OPT_SO | OPT_PR | OPT_CO;
    {
        int64_t tid[1]; float tlp[1];
        CallOpts pending = all_attached(lp, nb, ids, len);
        pending.tk = TopkAttach{8, tid, tlp, 20};
        CHECK(opts_set(pending) == (ALL | OPT_TK));
        unsigned refused = 0;
        CallOpts got = take_opts(pending, BEAM, OPT_FC, &refused);                          // a window beam search
        CHECK(refused == OPT_FC && got.tk.k == 0 && pending.tk.k == 8 && pending.tk.ids == tid && pending.tk.lp == tlp && pending.tk.ld == 20);
        got = take_opts(pending, OPT_LP, OPT_PR | OPT_CO | OPT_TK, &refused);                // a draft call
        CHECK(refused == OPT_TK && got.tk.k == 0 && got.lp.p == lp && pending.tk.k == 0 && opts_set(pending) == 0);
        pending.tk = TopkAttach{2, tid, tlp, 4};
        got = take_opts(pending, GREEDY | OPT_TK, 0, &refused);                              // a greedy call; score takes OPT_TK alone
        CHECK(refused == 0 && got.tk.k == 2 && got.tk.ld == 4 && opts_set(pending) == 0);
        CHECK(refused_message("greedy_draft", OPT_TK) == "greedy_draft: top-k alternatives are attached (gitcap_attach_top_logprobs), which this call does not take");
    }
    return 0;
}

// The student's record (StudentOpts) under the same take_opts: one row per family of gitcap_student_* entry points -- what it takes,
// what it refuses, what of five attachments is reported as refused and what stays pending behind it.
static int student_opts_test() {
    float lp[1], tlp[1]; int64_t tid[1]; const int64_t ids[1] = {0}; const int32_t len[1] = {1};
    const unsigned ALL = OPT_LP | OPT_TK | OPT_CO | OPT_PR | OPT_FC, GREEDY = OPT_LP | OPT_TK | OPT_CO | OPT_PR, DRAFT = OPT_PR | OPT_CO | OPT_TK;
    struct Row { unsigned take, refuse, refused, left; } rows[] = {
        {GREEDY | OPT_FC, 0, 0, 0},                         // student_greedy
        {GREEDY, OPT_FC, OPT_FC, 0},                        // student_window_greedy, _partial
        {OPT_LP | OPT_FC, DRAFT, DRAFT, 0},                 // student_greedy_draft
        {OPT_LP, OPT_FC | DRAFT, OPT_FC | DRAFT, 0},        // student_window_greedy_draft
        {GREEDY, OPT_FC, OPT_FC, 0},                        // student_pool_greedy
        {OPT_FC | OPT_CO | OPT_PR, 0, 0, OPT_LP | OPT_TK},  // student_beam_search
        {OPT_CO | OPT_PR, OPT_FC, OPT_FC, OPT_LP | OPT_TK}, // student_window_beam_search
        {OPT_TK, 0, 0, ALL & ~OPT_TK},                      // student_score
        {OPT_FC, 0, 0, ALL & ~OPT_FC},                      // student_set_memory
        {0, OPT_FC, OPT_FC, ALL & ~OPT_FC},                 // student_window_reset, _push, student_pool_reset, _push
        {0, 0, 0, ALL},                                     // student_pool_drop, _counts, _attention, _forward_decoder
    };
    for (const Row& r : rows) {
        StudentOpts pending;
        CHECK(opts_set(pending) == 0);
        pending.lp = LpAttach{lp, 8};
        pending.tk = TopkAttach{8, tid, tlp, 20};
        pending.co = ConsOpt{true, 2, 0, len, 1};
        pending.pr = PromptArgs{ids, 4, len, 1, 3};
        pending.fc.assign(300, 7);                          // more clips than RaggedCounts holds
        CHECK(opts_set(pending) == ALL);
        unsigned refused = 99;
        const StudentOpts got = take_opts(pending, r.take, r.refuse, &refused);
        CHECK(refused == r.refused && opts_set(got) == r.take && opts_set(pending) == r.left);
        if (r.take & OPT_FC) CHECK(got.fc.size() == 300 && got.fc[299] == 7);
        if (r.take & OPT_TK) CHECK(got.tk.k == 8 && got.tk.ids == tid && got.tk.lp == tlp && got.tk.ld == 20);
        if (r.left & OPT_LP) CHECK(pending.lp.p == lp && pending.lp.ld == 8);
        if (r.left & OPT_TK) CHECK(pending.tk.k == 8 && pending.tk.ld == 20);
        if (r.left & OPT_CO) CHECK(pending.co.on && pending.co.ngram == 2 && pending.co.suppress == len);
        if (r.left & OPT_PR) CHECK(pending.pr.ids == ids && pending.pr.max_len == 3);
        if (r.left & OPT_FC) CHECK(pending.fc.size() == 300 && pending.fc[0] == 7);
        // a second call finds nothing to take or refuse, and what stayed pending is intact
        (void)take_opts(pending, r.take, r.refuse, &refused);
        CHECK(refused == 0 && opts_set(pending) == r.left);
    }
    // the search part (gitcap_student_attach_search, OPT_SO): the beam family takes it, the greedy family, the drafts, score and
    // attention refuse and consume it, everything else leaves it pending; it combines with counts, constraints and a prompt
    float sc[1]; int32_t ln[1];
    struct SoRow { unsigned take, refuse, refused; bool left; } so_rows[] = {
        {OPT_FC | OPT_CO | OPT_PR | OPT_SO, 0, 0, false},           // student_beam_search
        {OPT_CO | OPT_PR | OPT_SO, OPT_FC, OPT_FC, false},          // student_window_beam_search, student_pool_beam_search
        {GREEDY | OPT_FC, OPT_SO, OPT_SO, false},                   // student_greedy
        {GREEDY, OPT_FC | OPT_SO, OPT_FC | OPT_SO, false},          // student_window_greedy, _partial, student_pool_greedy
        {OPT_LP | OPT_FC, DRAFT | OPT_SO, OPT_PR | OPT_CO | OPT_SO, false},     // student_greedy_draft
        {OPT_TK, OPT_SO, OPT_SO, false},                            // student_score
        {0, OPT_SO, OPT_SO, false},                                 // student_attention
        {OPT_FC, 0, 0, true},                                       // student_set_memory
        {0, OPT_FC, OPT_FC, true},                                  // the resets and pushes
    };
    for (const SoRow& r : so_rows) {
        StudentOpts pending;
        pending.se = StudentSearch{true, 2, 0.6f, 3, 1.3f, sc, ln};
        pending.co = ConsOpt{true, 2, 0, len, 1};
        pending.pr = PromptArgs{ids, 4, len, 1, 3};
        pending.fc.assign(3, 2);
        CHECK(opts_set(pending) == (OPT_SO | OPT_CO | OPT_PR | OPT_FC));
        unsigned refused = 99;
        const StudentOpts got = take_opts(pending, r.take, r.refuse, &refused);
        CHECK(refused == r.refused && ((opts_set(pending) & OPT_SO) != 0) == r.left);
        if (r.take & OPT_SO)
            CHECK(got.se.on && got.se.n == 2 && got.se.length_penalty == 0.6f && got.se.pn == 3 && got.se.rp == 1.3f && got.se.scores == sc &&
                  got.se.lengths == ln && got.co.on && got.pr.ids == ids);
        else
            CHECK(!got.se.on && got.se.scores == nullptr);
        if (r.left) CHECK(pending.se.on && pending.se.n == 2 && pending.se.scores == sc && pending.se.lengths == ln);
        (void)take_opts(pending, r.take, r.refuse, &refused);      // one-shot: nothing of it is found again
        CHECK((refused & OPT_SO) == 0 && ((opts_set(pending) & OPT_SO) != 0) == r.left);
    }
    return 0;
}

int main() {
    if (topk_opts_test() || student_opts_test()) return 1;
    // e4m3: every finite code round-trips through value -> exact code
    for (int code = 0; code < 256; ++code) {
        const float v = host_e4m3_value(code);
        if (std::isnan(v)) { CHECK((code & 0x7f) == 0x7f); continue; }
        CHECK(host_e4m3_exact(v) == code);
    }
    CHECK(host_e4m3_exact(448.f) == 0x7e && host_e4m3_exact(449.f) == -1 && host_e4m3_exact(0.3f) == -1);
    CHECK(host_e4m3_exact(std::ldexp(1.f, -9)) == 1 && host_e4m3_exact(std::ldexp(1.f, -10)) == -1);
    CHECK(host_e4m3_exact(INFINITY) == -1 && host_e4m3_exact(NAN) == -1);
    // bf16 rounding: ties to even, NaN preserved
    CHECK(host_f2bf(1.0f) == 0x3f80 && host_f2bf(-2.0f) == 0xc000);
    { uint32_t u = 0x3f808000u; float f; memcpy(&f, &u, 4); CHECK(host_f2bf(f) == 0x3f80); }     // tie -> even (down)
    { uint32_t u = 0x3f818000u; float f; memcpy(&f, &u, 4); CHECK(host_f2bf(f) == 0x3f82); }     // tie -> even (up)
    CHECK((host_f2bf(NAN) & 0x7fc0) == 0x7fc0);
    // row quantisation: values that ARE e4m3 x 2^k encode exactly into a buffer of exactly `cols` bytes; others are refused
    std::mt19937 rng(7);
    for (int trial = 0; trial < 200; ++trial) {
        const int cols = 1 + (int)(rng() % 97), k = (int)(rng() % 21) - 10;
        std::vector<float> row(cols);
        for (auto& v : row) {
            int code;
            do { code = (int)(rng() & 0xff); } while ((code & 0x7f) == 0x7f);
            v = std::ldexp(host_e4m3_value(code), k);
        }
        row[rng() % cols] = std::ldexp(448.f, k);                     // pin the row maximum: the scale must come out as 2^k
        const float scale = host_e4m3_row_scale(row.data(), cols);
        CHECK(scale == std::ldexp(1.f, k));
        std::vector<uint8_t> q(cols);                                 // exact size: an overrun is an ASan report
        CHECK(host_e4m3_encode_row(row.data(), cols, scale, q.data()));
        for (int i = 0; i < cols; ++i) CHECK(host_e4m3_value(q[i]) * scale == row[i]);
        row[0] = 0.3f * scale;
        CHECK(!host_e4m3_encode_row(row.data(), cols, scale, q.data()));
    }
    { std::vector<float> z(5, 0.f); CHECK(host_e4m3_row_scale(z.data(), 5) == 1.f); }
    // canonical tensor table: GIT-base has 12 encoder + 6 decoder layers worth of entries, names unique
    gitcap_config c{};
    c.image_size = 224; c.patch_size = 16; c.enc_width = 768; c.enc_layers = 12; c.enc_heads = 12; c.enc_ffn = 3072;
    c.dec_width = 768; c.dec_layers = 6; c.dec_heads = 12; c.dec_ffn = 3072; c.vocab_size = 30522; c.max_text_pos = 1024; c.num_frames = 6;
    std::vector<std::pair<std::string, std::vector<int64_t>>> shapes;
    expected_shapes(c, shapes);
    std::set<std::string> names;
    int gemm_w = 0;
    for (auto& kv : shapes) { names.insert(kv.first); gemm_w += is_gemm_weight(kv.first); CHECK(!kv.second.empty()); }
    CHECK(names.size() == shapes.size() && shapes.size() == 7 + 12 * 12 + 1 + 4 + 4 + 6 * 12 + 2);
    CHECK(gemm_w == 1 + 12 * 4 + 1 + 6 * 4 + 1);
    CHECK(!is_gemm_weight("enc.L0.qkv.b") && !is_gemm_weight("w") && is_gemm_weight("dec.L5.ao.w"));
    // tensor lookup of the loaders: unknown name, rank mismatch, shape mismatch (each with the caller's prefix), and a hit
    {
        std::map<std::string, DevTensor> table;
        for (auto& kv : shapes) table[kv.first].shape = kv.second;
        std::string err;
        const int64_t ok2[2] = {768, 768}, bad2[2] = {768, 767};
        CHECK(!find_tensor(table, "dec.L9.ao.w", ok2, 2, "load_tensor", err) && err == "load_tensor: unknown tensor 'dec.L9.ao.w'");
        CHECK(!find_tensor(table, "dec.L5.ao.w", ok2, 1, "student_load_tensor", err) && err == "student_load_tensor: rank mismatch for dec.L5.ao.w");
        CHECK(!find_tensor(table, "dec.L5.ao.w", bad2, 2, "tinyvit_load_tensor", err) && err == "tinyvit_load_tensor: shape mismatch for dec.L5.ao.w");
        CHECK(find_tensor(table, "dec.L5.ao.w", ok2, 2, "load_tensor", err) == &table["dec.L5.ao.w"]);
    }
    // tickets: four slots, a ticket is waitable until its slot is handed on
    CHECK(ticket_slot(5, 4) == 1 && ticket_waitable(5, 6, 4) && ticket_waitable(2, 6, 4) && !ticket_waitable(1, 6, 4));
    CHECK(!ticket_waitable(6, 6, 4) && !ticket_waitable(-1, 6, 4));
    // a failed exchange with tickets 3, 4, 5 in flight (next_ticket 6): all of them are refused from then on, ticket 6 (submitted
    // afterwards, on the unfused launches) is not; a second failure later moves the mark up
    {
        int upto = 0;
        CHECK(!ticket_poisoned(5, upto));
        upto = poison_mark(6);
        CHECK(ticket_poisoned(3, upto) && ticket_poisoned(5, upto) && !ticket_poisoned(6, upto) && ticket_waitable(5, 7, 4));
        upto = poison_mark(9);
        CHECK(ticket_poisoned(8, upto) && !ticket_poisoned(9, upto));
    }
    // window ring: a push of n entries from every head splits into the run up to the wrap and the remainder from slot 0, the
    // head moves by n modulo the slots, the count saturates, and emptying the ring keeps its size
    for (int F = 1; F <= 8; ++F)
        for (int head = 0; head < F; ++head)
            for (int n = 1; n <= F; ++n) {
                RingCursor r;
                r.reset(F);
                CHECK(r.slots == F && r.head == 0 && r.count == 0 && !r.full());
                for (int i = 0; i < head; ++i) r.push(1);
                CHECK(r.head == head && r.count == head && r.full() == (head == F));
                const int n1 = r.first_run(n), n2 = n - n1;
                CHECK(n1 >= 1 && n2 >= 0 && n1 + n2 == n && head + n1 <= F && (n2 == 0 || head + n1 == F) && n2 <= head);
                r.push(n);
                CHECK(r.head == (head + n1) % F + n2 && r.head < F && r.count == std::min(head + n, F) && r.full() == (head + n >= F));
                for (int i = 0; i < F; ++i) r.push(1);                    // F single pushes: the head is back where it was, the ring full
                CHECK(r.head == (head + n) % F && r.count == F && r.full());
                r.clear();
                CHECK(r.slots == F && r.count == 0 && !r.full() && r.head == (head + n) % F);
                r.reset(F);
                for (int i = 0; i < F; ++i) r.push(1);
                CHECK(r.head == 0 && r.full());
            }
    { RingCursor r; CHECK(!r.full()); }
    // residual + LayerNorm GEMM: every tile exactly once, a row block's tiles = consecutive workgroups of one XCD
    for (int ntn = 1; ntn <= 4; ++ntn)
        for (int nrb = 1; nrb <= 300; ++nrb) {
            const int grid = ln_grid_size(nrb, ntn);
            std::vector<int> seen((size_t)nrb * ntn, -1);
            for (int b = 0; b < grid; ++b) {
                int tm = -1, tn = -1;
                if (!ln_tile_of_block(b, nrb, ntn, &tm, &tn)) continue;
                CHECK(tm >= 0 && tm < nrb && tn >= 0 && tn < ntn && seen[(size_t)tm * ntn + tn] < 0);
                seen[(size_t)tm * ntn + tn] = b;
            }
            for (int tm = 0; tm < nrb; ++tm)
                for (int tn = 0; tn < ntn; ++tn) {
                    CHECK(seen[(size_t)tm * ntn + tn] >= 0);
                    if (tn) CHECK(seen[(size_t)tm * ntn + tn] == seen[(size_t)tm * ntn + tn - 1] + 8);   // same XCD, next in its sequence
                }
        }
    // the row-block map is used as soon as the grid exceeds the device's CUs (also on a partitioned device)
    CHECK(!ln_use_rowblock_map(74, 3) && ln_use_rowblock_map(148, 3));
    CHECK(ln_use_rowblock_map(74, 3, 128) && !ln_use_rowblock_map(40, 3, 128) && ln_use_rowblock_map(11, 3, 32));
    // exchange health: a clean word changes nothing; a raised one degrades the handle for good and is reported every time it is seen
    {
        ExchangeHealth hs;
        CHECK(!exchange_poll(hs, 0u) && !hs.degraded && hs.trips == 0);
        CHECK(exchange_poll(hs, 1u) && hs.degraded && hs.trips == 1);
        CHECK(!exchange_poll(hs, 0u) && hs.degraded && hs.trips == 1);          // the caller cleared the word: quiet again, still degraded
        CHECK(exchange_poll(hs, 7u) && hs.degraded && hs.trips == 2);
    }
    if (int rc = call_opts_test()) return rc;
    CHECK(pad_to(18912, 256) == 18944 && pad_to(256, 256) == 256 && pad_to(1, 16) == 16);
    std::puts("host_asan_test ok");
    return 0;
}
