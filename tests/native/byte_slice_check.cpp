// Host check of the 8x8 bit-matrix helpers behind k_om3wt's byte-sliced input
// staging and result pick-out (csrc/ba_bitslice.hpp):
//   1. transpose8x8 is its own inverse and equals a bit-by-bit transpose, on
//      random and on every single-bit matrix;
//   2. stage_load + stage_pack give byte k of the planes that stage_slice
//      (csrc/ba_wave.hpp) defines per trial: plane g < N = bit g of the faulty
//      mask (bits >= N ignored), OB = order byte == 1, OO = order byte == 2 over
//      all 256 byte values, VAL = the trial is inside the batch; a trial at or
//      beyond batch gives 0 in every plane.  Every valid count 0..8 of a lane,
//      on buffers of exactly `batch` elements at 4-byte / 1-byte alignment (the
//      sanitizer build catches any access outside them);
//   3. pick_out gives the per-trial decision word and outcome byte that phase 2
//      of wave_epilogue picks with bit(): dec bit 2b = A[b], bit 2b+1 = U[b]
//      (even L only), out bit k = outcome plane k; L = 9 and every even L,
//      every L up to 16 besides.
// Built as host code by tests/test_byte_slice.py (hipcc; no device needed).
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../byzantine-agreement_amd/csrc/ba_bitslice.hpp"

using namespace ba;

static long bad = 0, checks = 0;
#define CHECK(c, ...)                                    \
    do {                                                 \
        ++checks;                                        \
        if (!(c)) {                                      \
            if (++bad <= 10) std::printf(__VA_ARGS__);   \
        }                                                \
    } while (0)

static uint64_t naive_transpose(uint64_t x) {
    uint64_t r = 0;
    for (int row = 0; row < 8; ++row)
        for (int col = 0; col < 8; ++col)
            if ((x >> (8 * row + col)) & 1u) r |= 1ull << (8 * col + row);
    return r;
}

static void check_transpose(std::mt19937_64& rng) {
    for (int b = 0; b < 64; ++b) {
        const uint64_t x = 1ull << b;
        CHECK(transpose8x8(x) == naive_transpose(x), "transpose: single bit %d\n", b);
        CHECK(transpose8x8(~x) == naive_transpose(~x), "transpose: all but bit %d\n", b);
    }
    for (int rep = 0; rep < 200000; ++rep) {
        const uint64_t x = rng() & (rep % 3 == 0 ? rng() : ~0ull);
        const uint64_t t = transpose8x8(x);
        CHECK(t == naive_transpose(x), "transpose: %016llx\n", (unsigned long long)x);
        CHECK(transpose8x8(t) == x, "transpose twice: %016llx\n", (unsigned long long)x);
    }
}

template <int N, int G>
static void check_planes(const StagePlanes<N>& p, const uint32_t (&want)[N + 3], uint64_t i0, uint64_t batch) {
    if constexpr (G < N + 3) {
        CHECK(p.template plane<G>() == want[G], "stage N=%d plane %d i0=%llu batch=%llu: %02x want %02x\n", N,
              G, (unsigned long long)i0, (unsigned long long)batch, p.template plane<G>(), want[G]);
        check_planes<N, G + 1>(p, want, i0, batch);
    }
}

// the per-trial definition (stage_slice / stage_words in csrc/ba_wave.hpp)
template <int N>
static void check_stage_lane(const uint32_t* faulty, const uint8_t* order, uint64_t base, uint32_t off,
                             uint64_t batch) {
    const uint64_t i0 = base + off;
    uint32_t want[N + 3] = {};
    for (int t = 0; t < 8; ++t) {
        const uint64_t i = i0 + t;
        if (i >= batch) continue;
        const uint32_t fm = faulty[i], c = order[i];
        for (int g = 0; g < N; ++g) want[g] |= ((fm >> g) & 1u) << t;
        want[N] |= (c == 1u ? 1u : 0u) << t;
        want[N + 1] |= (c == 2u ? 1u : 0u) << t;
        want[N + 2] |= 1u << t;
    }
    const StagePlanes<N> p = stage_pack<N>(stage_load(faulty, order, base, off, batch));
    check_planes<N, 0>(p, want, i0, batch);
}

template <int N>
static void check_stage(std::mt19937_64& rng) {
    // every valid count 0..8 of the last lanes: batches 0..40 and 64..104 (the wave
    // based at trial 0 / 64) in buffers of exactly `batch` elements; the faulty
    // buffer is offset to every 4-byte phase of 16 and the order buffer to every
    // byte phase of 8
    for (uint64_t batch = 0; batch <= 104; batch += batch == 40 ? 24 : 1)
        for (int phase = 0; phase < 8; ++phase) {
            const uint64_t base = batch >= 64 ? 64 : 0;
            std::vector<uint32_t> fbuf(batch + (phase & 3));
            std::vector<uint8_t> obuf(batch + phase);
            uint32_t* f = fbuf.data() + (phase & 3);
            uint8_t* o = obuf.data() + phase;
            for (uint64_t i = 0; i < batch; ++i) {
                f[i] = (uint32_t)rng();  // bits >= N set
                o[i] = (uint8_t)(rng() % 4 == 0 ? rng() : rng() % 3);
            }
            for (uint32_t off = 0; off < 64; off += 8) check_stage_lane<N>(f, o, base, off, batch);
        }
    // all 256 order bytes in every trial position, masks all ones / only high bits
    std::vector<uint32_t> f(8);
    std::vector<uint8_t> o(8);
    for (int c = 0; c < 256; ++c)
        for (int t = 0; t < 8; ++t) {
            for (int k = 0; k < 8; ++k) {
                f[k] = k == t ? ~0u : ~0u << N;
                o[k] = (uint8_t)(k == t ? c : (c + 1 + k) & 0xff);
            }
            check_stage_lane<N>(f.data(), o.data(), 0, 0, 8);
        }
    for (int rep = 0; rep < 50000; ++rep) {
        for (int k = 0; k < 8; ++k) {
            f[k] = (uint32_t)rng();
            o[k] = (uint8_t)rng();
        }
        check_stage_lane<N>(f.data(), o.data(), 0, 0, 8);
    }
}

// wave_epilogue phase 2 per trial: bit() of the planes
template <int L>
static void check_pick(std::mt19937_64& rng) {
    for (int rep = 0; rep < 20000; ++rep) {
        uint32_t a[L], u[L], o[6];
        // only byte 0 counts: the rest is noise, as the complemented planes of
        // epilogue_core leave it
        const uint32_t noise = rep % 2 ? 0xffffff00u : 0u;
        for (int b = 0; b < L; ++b) {
            a[b] = (uint32_t)rng() & (0xffu | noise);
            u[b] = (uint32_t)rng() & (0xffu | noise);
        }
        for (int k = 0; k < 6; ++k) o[k] = (uint32_t)rng() & (0xffu | noise);
        if (rep < 8 * (L + 6)) {  // single planes
            for (int b = 0; b < L; ++b) a[b] = u[b] = 0;
            for (int k = 0; k < 6; ++k) o[k] = 0;
            const int pl = rep / 8;
            if (pl < L) a[pl] = 0xffu;
            else o[pl - L] = 0xffu;
        }
        const PickOut<L> p = pick_out<L>(a, u, o);
        for (int t = 0; t < 8; ++t) {
            uint32_t dec = 0, out = 0;
            for (int b = 0; b < L; ++b) {
                dec |= ((a[b] >> t) & 1u) << (2 * b);
                if (L % 2 == 0) dec |= ((u[b] >> t) & 1u) << (2 * b + 1);
            }
            for (int k = 0; k < 6; ++k) out |= ((o[k] >> t) & 1u) << k;
            const uint32_t got_out = ((t < 4 ? p.out_lo : p.out_hi) >> (8 * (t & 3))) & 0xffu;
            CHECK(p.dec[t] == dec, "pick L=%d trial %d: dec %08x want %08x\n", L, t, p.dec[t], dec);
            CHECK(got_out == out, "pick L=%d trial %d: out %02x want %02x\n", L, t, got_out, out);
        }
    }
}

template <int L>
static void check_pick_upto(std::mt19937_64& rng) {
    check_pick<L>(rng);
    if constexpr (L > 1) check_pick_upto<L - 1>(rng);
}

int main() {
    std::mt19937_64 rng(0xb17e5);
    check_transpose(rng);
    check_stage<10>(rng);
    check_stage<9>(rng);
    check_stage<13>(rng);
    check_pick_upto<16>(rng);
    std::printf("byte_slice_check: %ld checks, %ld bad\n", checks, bad);
    if (bad == 0) std::printf("byte_slice_check ok\n");
    return bad == 0 ? 0 : 1;
}
