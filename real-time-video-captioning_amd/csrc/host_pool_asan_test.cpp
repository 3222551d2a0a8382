// CPU-only driver of the stream pool's cursor arithmetic (host_logic.h: pool_push_slots, pool_push_commit, RingCursor::oldest) under
// AddressSanitizer + UBSan (`make asan-pool`): no HIP, no GPU.  A model that keeps every stream's tokens in a plain list says where
// each token must be and which are the last `slots` of a stream, oldest first.
#include "host_logic.h"

#include <cstdio>
#include <random>

#define CHECK(c) do { if (!(c)) { std::fprintf(stderr, "host_pool_asan_test: %s:%d: %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

// S streams of F slots driven by `pushes` random pushes; ring[row] = the serial number of the token the row holds
static int run(int S, int F, int pushes, unsigned seed) {
    std::mt19937 rng(seed);
    std::vector<RingCursor> cur((size_t)S);
    for (RingCursor& c : cur) c.reset(F);
    std::vector<std::vector<int>> model((size_t)S);
    std::vector<int> ring((size_t)S * F, -1);
    int serial = 0;
    for (int p = 0; p < pushes; ++p) {
        const int n = 1 + (int)(rng() % (unsigned)(2 * F + 3));
        std::vector<int32_t> ids((size_t)n), slot((size_t)n, -7);
        std::vector<int> per((size_t)S, 0);
        bool over = false;
        for (int i = 0; i < n; ++i) {
            ids[(size_t)i] = (int32_t)(rng() % (unsigned)S);
            over |= ++per[(size_t)ids[(size_t)i]] > F;
        }
        const std::vector<RingCursor> before = cur;
        int bad = -2;
        const int rc = pool_push_slots(cur, ids.data(), n, slot.data(), &bad);
        for (int s = 0; s < S; ++s)         // the plan changes no cursor, accepted or not
            CHECK(cur[(size_t)s].head == before[(size_t)s].head && cur[(size_t)s].count == before[(size_t)s].count);
        CHECK((rc == POOL_PUSH_OVER) == over);
        if (rc != POOL_PUSH_OK) {
            CHECK(bad >= 0 && bad < n);
            continue;
        }
        CHECK(bad == -1);
        std::vector<int> hit((size_t)S * F, 0);
        for (int i = 0; i < n; ++i) {       // inside its own stream's rows, and no row twice in one push
            const int row = slot[(size_t)i];
            CHECK(row >= ids[(size_t)i] * F && row < (ids[(size_t)i] + 1) * F);
            CHECK(hit[(size_t)row]++ == 0);
            ring[(size_t)row] = serial;
            model[(size_t)ids[(size_t)i]].push_back(serial++);
        }
        pool_push_commit(cur, ids.data(), n);
        for (int s = 0; s < S; ++s) {       // every stream holds its last min(count, F) tokens, oldest first from oldest()
            const RingCursor& c = cur[(size_t)s];
            const std::vector<int>& m = model[(size_t)s];
            const int held = (int)m.size() < F ? (int)m.size() : F;
            CHECK(c.count == held && c.full() == (held == F));
            if (!held) continue;
            CHECK(c.oldest() >= 0 && c.oldest() < F);
            for (int f = 0; f < held; ++f)
                CHECK(ring[(size_t)s * F + (size_t)((c.oldest() + f) % F)] == m[m.size() - (size_t)held + (size_t)f]);
        }
    }
    return 0;
}

int main() {
    // ids outside the pool are refused at the first of them, whatever came before
    {
        std::vector<RingCursor> cur(3);
        for (RingCursor& c : cur) c.reset(4);
        int32_t slot[4] = {0, 0, 0, 0};
        int bad = -2;
        const int32_t neg[3] = {0, -1, 2}, big[2] = {3, 0}, five[5] = {1, 1, 1, 1, 1};
        CHECK(pool_push_slots(cur, neg, 3, slot, &bad) == POOL_PUSH_BAD_ID && bad == 1);
        CHECK(pool_push_slots(cur, big, 2, slot, &bad) == POOL_PUSH_BAD_ID && bad == 0);
        int32_t slot5[5];
        CHECK(pool_push_slots(cur, five, 5, slot5, &bad) == POOL_PUSH_OVER && bad == 4);
        CHECK(pool_push_slots(cur, five, 4, slot5, &bad) == POOL_PUSH_OK && slot5[0] == 4 && slot5[3] == 7);
        // an empty pool refuses every id
        std::vector<RingCursor> none;
        CHECK(pool_push_slots(none, big, 1, slot, &bad) == POOL_PUSH_BAD_ID && bad == 0);
    }
    if (run(1, 1, 50, 1) || run(5, 6, 400, 2) || run(3, 64, 200, 3) || run(4096, 2, 60, 4) || run(7, 5, 400, 5)) return 1;
    std::puts("host_pool_asan_test ok");
    return 0;
}
