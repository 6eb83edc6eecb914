// Host check of k_om3wt's per-task helpers (csrc/ba_om3_task.hpp):
//   1. om3_lane_tables<S, CP>(la) equals, byte by byte, the two tables that
//      Om3LaneOffsets (csrc/ba_wave.hpp) defines per member:
//        mem[a] = 8 (a + (a >= la))      r2t[d] = 8 CP (d >= la) ? : 0
//      packed one per byte from byte 0, zero above byte S - 1, for every la in
//      0..S (n = 10: S = 7, CP = 9, la = 0..7) and for the other S <= 7;
//   2. Om3RootHalves<L, W, LP>: over its trips the 64 lanes' units cover every
//      (word, receiver, half) of the W L root columns exactly once, a unit's
//      source is the first dword of that half of R1T[w][col][0] and its
//      destination that half of the dense image a[w L + col]; no unit reads or
//      writes outside R1T[W][L][LP] and a[W L] (the sanitizer build sees any);
//   3. run() on random R1T images gives the strict majority of the L inputs of
//      every column, bit for bit what roots_r1t's 64-bit count gives (a count
//      over single bits here), and leaves a sentinel behind a[] untouched;
//   4. mul_u24 and lds_at on the host are the plain product and byte offset.
// Built as host code by tests/test_om3_task.py (hipcc; no device needed).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../byzantine-agreement_amd/csrc/ba_om3_task.hpp"

using namespace ba;

static long bad = 0, checks = 0;
#define CHECK(c, ...)                                    \
    do {                                                 \
        ++checks;                                        \
        if (!(c)) {                                      \
            if (++bad <= 10) std::printf(__VA_ARGS__);   \
        }                                                \
    } while (0)

template <int S, int CP>
static void check_tables() {
    for (uint32_t la = 0; la <= (uint32_t)S; ++la) {
        const Om3LaneTables t = om3_lane_tables<S, CP>(la);
        for (int a = 0; a < 8; ++a) {
            // the lambdas of Om3LaneOffsets, as LaneBytes packs them
            const uint32_t mem = a < S ? 8u * (a + ((uint32_t)a >= la ? 1u : 0u)) : 0u;
            const uint32_t r2t = a < S ? ((uint32_t)a >= la ? 8u * CP : 0u) : 0u;
            CHECK(((t.mem >> (8 * a)) & 0xffu) == mem, "mem S=%d CP=%d la=%u a=%d: %llx\n", S, CP, la, a,
                  (unsigned long long)t.mem);
            CHECK(((t.r2t >> (8 * a)) & 0xffu) == r2t, "r2t S=%d CP=%d la=%u d=%d: %llx\n", S, CP, la, a,
                  (unsigned long long)t.r2t);
        }
    }
}

template <int L, int W, int LP>
static void check_roots(std::mt19937_64& rng) {
    using R = Om3RootHalves<L, W, LP>;
    // ---- the mapping ------------------------------------------------------------
    std::vector<int> seen(2 * W * L, 0);
    static_for_h<0, (int)R::TRIPS>([&](auto t) {
        constexpr uint32_t T = (uint32_t)t();
        for (uint32_t lane = 0; lane < 64; ++lane) {
            if (!R::template live<T>(lane)) continue;
            const uint32_t src = R::src(lane) + T * R::SRC_TRIP, dst = R::dst(lane) + T * R::DST_TRIP;
            const uint32_t h = 64 * T + lane, col = h >> 1, half = h & 1u;  // col = w L + receiver
            CHECK(col < (uint32_t)(W * L), "unit %u beyond the columns\n", h);
            if (col < (uint32_t)(W * L)) ++seen[2 * col + half];
            CHECK(src == 8u * LP * col + 4u * half, "src trip %u lane %u: %u\n", T, lane, src);
            CHECK(dst == 8u * col + 4u * half, "dst trip %u lane %u: %u\n", T, lane, dst);
            CHECK(src + 8u * (L - 1) + 4u <= 8u * W * L * LP, "src trip %u lane %u outside R1T\n", T, lane);
            CHECK(dst + 4u <= 8u * W * L, "dst trip %u lane %u outside the image\n", T, lane);
        }
    });
    for (int w = 0; w < W; ++w)
        for (int b = 0; b < L; ++b)
            for (int half = 0; half < 2; ++half)
                CHECK(seen[2 * (w * L + b) + half] == 1, "(word %d, receiver %d, half %d) covered %d times\n", w,
                      b, half, seen[2 * (w * L + b) + half]);
    // ---- the majorities ---------------------------------------------------------
    const uint64_t sentinel = 0xA5A55A5AC3C33C3Cull;
    for (int rep = 0; rep < 200; ++rep) {
        // exactly sized buffers: the sanitizer build catches any access outside them
        std::vector<uint64_t> r1t((size_t)W * L * LP), a((size_t)W * L + 1, sentinel);
        for (auto& x : r1t) x = rep % 4 == 0 ? rng() & rng() : (rep % 4 == 1 ? rng() | rng() : rng());
        for (uint32_t lane = 0; lane < 64; ++lane) R::run(r1t.data(), a.data(), lane);
        for (int c = 0; c < W * L; ++c) {
            uint64_t want = 0;
            for (int bit = 0; bit < 64; ++bit) {
                int n = 0;
                for (int j = 0; j < L; ++j) n += (int)((r1t[(size_t)c * LP + j] >> bit) & 1u);
                if (n >= L / 2 + 1) want |= 1ull << bit;
            }
            CHECK(a[c] == want, "majority rep %d column %d: %016llx want %016llx\n", rep, c,
                  (unsigned long long)a[c], (unsigned long long)want);
        }
        CHECK(a[(size_t)W * L] == sentinel, "rep %d: store behind the image\n", rep);
    }
}

int main() {
    std::mt19937_64 rng(0x0B3ull);
    check_tables<7, 9>();  // n = 10
    check_tables<7, 8>();
    check_tables<5, 7>();
    check_tables<3, 5>();
    check_tables<1, 3>();
    check_roots<9, 8, 9>(rng);   // n = 10: 144 units, three trips, the last of 16 lanes
    check_roots<9, 8, 10>(rng);  // a padded R1T row
    check_roots<7, 10, 7>(rng);
    check_roots<5, 16, 5>(rng);  // 160 units
    check_roots<3, 3, 3>(rng);   // fewer units than lanes
    for (uint32_t a = 0; a < 64; ++a) CHECK(mul_u24(a, 104u) == a * 104u, "mul_u24 %u\n", a);
    uint64_t words[4] = {0, 0, 0, 0};
    CHECK(lds_at(words, 24) == words + 3, "lds_at\n");
    CHECK(lds_at((const uint64_t*)words, 8) == words + 1, "lds_at const\n");
    std::printf("%ld checks, %ld bad\n", checks, bad);
    if (bad == 0) std::printf("om3_task_check ok\n");
    return bad != 0;
}
