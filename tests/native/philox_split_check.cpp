// Host check of the split of Philox4x32-10 rounds 0-1 that k_om3wt's pair table
// uses (ba_device.hpp: philox_pair_entry, philox_word_consts, philox_finish01):
// for a counter {pair, level, gw_lo, gw_hi} the pair-only entry, finished with
// the per-(word, level) constants, must be philox10's state after two rounds,
// and running the remaining eight rounds on it must give philox10's output.
// Random pairs, words, keys; levels 0-5; gw_hi in {0, 1, random}.  Built as
// host code by tests/test_philox_split.py (hipcc; no device needed).
#include <cstdio>
#include <random>

#include "../../byzantine-agreement_amd/csrc/ba_device.hpp"

using namespace ba;

// rounds FROM..9 of philox10 on a state whose first FROM rounds are done
static P4 rounds_from(int from, P4 c, uint32_t k0, uint32_t k1) {
    k0 += (uint32_t)from * 0x9E3779B9u;
    k1 += (uint32_t)from * 0xBB67AE85u;
    for (int i = from; i < 10; ++i) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c.x, p1 = (uint64_t)0xCD9E8D57u * c.z;
        c = P4{(uint32_t)(p1 >> 32) ^ c.y ^ k0, (uint32_t)p1, (uint32_t)(p0 >> 32) ^ c.w ^ k1,
               (uint32_t)p0};
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

static bool same(const P4& a, const P4& b) {
    return a.x == b.x && a.y == b.y && a.z == b.z && a.w == b.w;
}

int main() {
    std::mt19937_64 rng(0x5eed0a11);
    long bad = 0, n = 0;
    for (int rep = 0; rep < 40000; ++rep) {
        const uint32_t k0 = (uint32_t)rng(), k1 = (uint32_t)rng();
        // small pairs (what the kernels draw), pairs near 2^32 and random ones
        const uint32_t pair = rep % 3 == 0 ? (uint32_t)(rng() % 2000) : (rep % 3 == 1 ? ~(uint32_t)(rng() % 2000) : (uint32_t)rng());
        const uint32_t gw_lo = rep % 5 == 0 ? ~(uint32_t)(rng() % 16) : (uint32_t)rng();
        const uint32_t hsel = rep % 4;
        const uint32_t gw_hi = hsel == 0 ? 0u : (hsel == 1 ? 1u : (uint32_t)rng());
        for (uint32_t level = 0; level <= 5; ++level, ++n) {
            const P4 want = philox10(P4{pair, level, gw_lo, gw_hi}, k0, k1);
            const PhiloxPairEntry e = philox_pair_entry(pair, gw_hi, k1);
            const PhiloxWordConsts wc = philox_word_consts(level, gw_lo, k0, k1);
            const P4 s2 = philox_finish01(e, wc);
            // the entry may depend on nothing but (pair, gw_hi, k1): a second word
            // and level with the same entry must come out right too
            const uint32_t gw2 = (uint32_t)rng(), lv2 = (level + 1 + (uint32_t)(rng() % 5)) % 6;
            const P4 want2 = philox10(P4{pair, lv2, gw2, gw_hi}, k0, k1);
            const P4 got2 = rounds_from(2, philox_finish01(e, philox_word_consts(lv2, gw2, k0, k1)), k0, k1);
            if (!same(rounds_from(2, s2, k0, k1), want) || !same(got2, want2)) {
                if (++bad < 5)
                    printf("mismatch pair=%u level=%u gw=%08x:%08x key=%08x:%08x\n", pair, level,
                           gw_hi, gw_lo, k1, k0);
            }
        }
    }
    // the reference rounds above are philox10's own: zero rounds done = the call
    for (int rep = 0; rep < 1000; ++rep, ++n) {
        const P4 c{(uint32_t)rng(), (uint32_t)rng(), (uint32_t)rng(), (uint32_t)rng()};
        const uint32_t k0 = (uint32_t)rng(), k1 = (uint32_t)rng();
        if (!same(rounds_from(0, c, k0, k1), philox10(c, k0, k1))) ++bad;
    }
    printf("philox_split_check %s (%ld cases, %ld mismatches)\n", bad ? "FAILED" : "ok", n, bad);
    return bad ? 1 : 0;
}
