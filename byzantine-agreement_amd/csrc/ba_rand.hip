// ba_rand.hip -- randomized agreement, Ben-Or rounds with a local or a common coin
// (docs/SEMANTICS.md §13), one 64-trial word per wave (k_rand, gfx950).
//
// k_king3's frame (ba_king3.hip) carries over: one preference plane per general,
// lane (i, s) = i + 32 s is recipient i < n with sender slice s, lane b is trial b
// for the inputs, `decided` and the epilogue; the walk over the sender pairs, its
// Philox calls and the tallies are ba_king_common.hpp's king3_round / king3_merge,
// under this protocol's tag 256.  Every general also keeps the planes D (decided,
// sticky) and V (the value it decided).  A phase has three steps:
//   report   c1 = the attack votes shown; proposals A = [c1 >= T] and
//            R = [c1 <= n - T], T = (n + m) / 2 + 1 (2c > n + m; never both)
//   propose  two sender planes A[j], R[j] in LDS; a faulty j shows the coin as A and
//            its complement as R.  One walk feeds d1 and d0; v = retreat if
//            d0 >= m + 1, else attack if d1 >= m + 1; where v exists x = v, and
//            where also d_v >= T and D is clear, D is set and V = v
//   toss     where v does not exist, x = the coin: BA_RAND_LOCAL general i's own call
//            (sender i to recipient i, a slot no message uses), BA_RAND_COMMON one
//            call for the word; neither is drawn when no trial of the word needs it
// Per wave, in LDS (4,648 B; four waves per block, no block barrier):
//   F[j], pref[j], pa[j], pr[j], part[p][l]   as in k_king3
//   D[j], V[j]       general j's decision planes, read and written by its own lanes
//                    around the propose round's end
//   fm[b], oc[b]     trial b's inputs, kept for the epilogue
// D, V and the inputs live in LDS and not in registers because the walk's four
// interleaved Philox calls set the kernel's register peak: held across them they
// cost the COIN kernels their third wave per SIMD (176 against 166 to 169 VGPRs).
//   chk[5]   once per phase, ORed over the generals' lanes and read with lane =
//            trial: loyal and decided attack / retreat, loyal with D set and
//            x != V, loyal with D clear, any general with D clear
//
// Wave-uniform shortcuts, invisible in the results: king3_round's undrawn call
// groups, BA_KING_SPLIT drawing no message coins, the undrawn toss, and the early
// finish: when at the end of a phase every trial of the word is in bound
// (|F| <= m, n > 3m) and every one of the n generals, the faulty ones' honest state
// included, has D set, every x equals the one decided value and stays there (§13),
// so the word's remaining phases are skipped.  Beyond the bound there is no such
// fixed point: a word with one out-of-bound trial runs all its phases.
#include "ba_king_common.hpp"

namespace ba {

constexpr uint32_t kRandTag = 256;   // Philox ctr word 1 of step q: kRandTag + q
constexpr int kRandThreads = 256;    // four independent waves

struct RandWave {
    uint64_t F[kMaxN];
    uint64_t pref[kMaxN];
    uint64_t pa[kMaxN], pr[kMaxN];
    uint64_t part[kKing3PartPlanes][64];
    uint64_t D[kMaxN], V[kMaxN];
    uint64_t chk[5];
    uint32_t fm[64], oc[64];
};

template <bool GEN, bool COIN, bool COMMON>
__global__ __launch_bounds__(kRandThreads) void k_rand(uint32_t n, uint32_t m, uint32_t phases,
                                                       uint64_t seed, GenSpec gen,
                                                       uint64_t first_trial, uint64_t batch,
                                                       const uint32_t* __restrict__ faulty,
                                                       const uint8_t* __restrict__ order,
                                                       uint64_t* __restrict__ decisions,
                                                       uint8_t* __restrict__ outcome,
                                                       uint8_t* __restrict__ decided,
                                                       uint64_t* __restrict__ counters, Sink sk) {
    __shared__ RandWave lds[kRandThreads / 64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t i = lane & 31u, sl = lane >> 5;
    RandWave& s = lds[wv];
    const uint32_t all = general_mask(n);
    const uint32_t npairs = (n + 1) / 2;
    // 2c > n + m  <=>  c >= T (T <= 22; beyond n nobody proposes); d > m  <=>  d >= Tm
    const uint32_t T = (n + m) / 2 + 1, Tm = m + 1;
    const uint64_t words = (batch + 63) / 64;
    const uint32_t nwaves = gridDim.x * (kRandThreads / 64), gwave = blockIdx.x * (kRandThreads / 64) + wv;
    uint64_t mine = 0;
    for (uint64_t w = gwave; w < words; w += nwaves) {
        const uint64_t t = w * 64 + lane, gw = (first_trial >> 6) + w;
        const bool live = t < batch;
        uint32_t fm, oc;
        trial_inputs<GEN>(live, n, all, seed, gen, first_trial, t, faulty, order, fm, oc);
        // planes of the word
        const uint64_t OB = __ballot(oc == 1);
        // every trial of the word in bound (a trial past the batch has nobody faulty)
        const bool inb_all = n > 3 * m && __ballot((uint32_t)__popc(fm) > m) == 0;
        uint64_t myF = 0, F0 = 0;
        for (uint32_t g = 0; g < n; ++g) {
            const uint64_t pl = faulty_plane(fm, g);
            if (g == 0) F0 = pl;
            if (i == g) myF = pl;
        }
        wave_sync();  // the previous word's epilogue has read pref
        s.fm[lane] = fm, s.oc[lane] = oc;
        uint32_t st = 255;  // decided so far (lane = trial)
        if (lane < 32) {
            s.F[lane] = myF;
            s.D[lane] = 0;
            s.V[lane] = 0;
        }
        // round 0: the commander sends
        uint64_t pref = OB;
        if (F0 != 0) {
            const uint64_t c = king_one_coin<COIN, kRandTag>(0, i, 0, gw, seed);
            if (i != 0) pref = (OB & ~F0) | (F0 & c);
        }
        if (i >= n) pref = 0;
        for (uint32_t p = 1; p <= phases; ++p) {
            wave_sync();
            if (lane < 32) s.pref[lane] = pref;
            wave_sync();
            // report q = 3p - 2
            uint64_t A, R;
            {
                Tally3 tv, unused;
                king3_round<kRandTag, COIN, false>(s, i, sl, n, npairs, 3 * p - 2, gw, seed, pref, 0, tv,
                                                   unused);
                const auto c1 = king3_merge(s, lane, tv);
                A = c1.ge(T);
                R = T <= n ? ~c1.ge(n - T + 1) : 0ull;  // c0 >= T  <=>  c1 <= n - T
            }
            if (i >= n) A = R = 0;  // a general that is not there proposes nothing
            if (lane < 32) {
                s.pa[lane] = A;
                s.pr[lane] = R;
            }
            wave_sync();
            // propose q = 3p - 1
            uint64_t v0, v1, D, V;
            {
                Tally3 ta, tr;
                king3_round<kRandTag, COIN, true>(s, i, sl, n, npairs, 3 * p - 1, gw, seed, A, R, ta, tr);
                const auto d1 = king3_merge(s, lane, ta);
                const uint64_t x1 = d1.ge(Tm), s1 = d1.ge(T);
                const auto d0 = king3_merge(s, lane, tr);
                v0 = d0.ge(Tm);
                v1 = x1 & ~v0;
                D = s.D[i], V = s.V[i];
                const uint64_t fresh = ((v0 & d0.ge(T)) | (v1 & s1)) & ~D;
                V |= fresh & v1;
                D |= fresh;
                if (i >= n) D = V = 0;
                if (lane < 32) {
                    s.D[lane] = D;
                    s.V[lane] = V;
                }
            }
            // toss q = 3p: only where v does not exist
            const uint64_t none = ~(v0 | v1);
            uint64_t c = 0;
            if (__ballot(i < n && none != 0) != 0)
                c = COMMON ? king_one_coin<true, kRandTag>(0, 0, 3 * p, gw, seed)
                           : king_one_coin<true, kRandTag>(i, i, 3 * p, gw, seed);
            pref = v1 | (none & c);
            if (i >= n) pref = 0;
            // end of the phase: `decided` and the early finish
            if (decided || inb_all) {
                wave_sync();
                if (lane < 5) s.chk[lane] = 0;
                wave_sync();
                if (lane < n) {
                    lds_or(&s.chk[4], ~D);
                    if (decided) {
                        const uint64_t loyal = ~s.F[lane], LD = loyal & D;
                        lds_or(&s.chk[0], LD & V);
                        lds_or(&s.chk[1], LD & ~V);
                        lds_or(&s.chk[2], LD & (pref ^ V));
                        lds_or(&s.chk[3], loyal & ~D);
                    }
                }
                wave_sync();
                if (decided) {
                    const uint64_t a1 = s.chk[0], a0 = s.chk[1];
                    // two decided values; a decided general moved; a loyal commander's order not kept
                    const uint64_t bad = (a1 & a0) | s.chk[2] | (~F0 & ((a1 & ~OB) | (a0 & OB)));
                    if ((bad >> lane) & 1ull) st = 254;
                    else if (st == 255 && ((s.chk[3] >> lane) & 1ull) == 0) st = p;
                }
                if (inb_all && __ballot(s.chk[4] != 0) == 0) break;  // early finish
            }
        }
        // epilogue, lane = trial: decisions, quorum, flags
        wave_sync();
        if (lane < 32) s.pref[lane] = pref;
        wave_sync();
        uint32_t Adec = 0;
        for (uint32_t r = 1; r < n; ++r) Adec |= lane_bit(&s.pref[r], lane) << r;
        TrialResult res = trial_result(n, 0, s.fm[lane], s.oc[lane], Adec, 0);
        // in-bound is this protocol's: |F| <= m and n > 3m
        res.out = (res.out & ~32u) | ((res.nf <= m && n > 3 * m) ? 32u : 0u);
        if (live) {
            if (decisions) decisions[t] = res.dec;
            if (outcome) outcome[t] = (uint8_t)res.out;
            if (decided) decided[t] = (uint8_t)st;
        }
        lane_counts_add<false>(live, res, lane, mine);
    }
    sink_counters(lane, mine, gwave, nwaves, counters, sk);
}

// Resident blocks per CU of one instantiation (its registers decide), asked of
// the runtime once.
template <bool GEN, bool COIN, bool COMMON>
static uint32_t rand_blocks_per_cu() {
    static const uint32_t v = [] {
        int o = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, k_rand<GEN, COIN, COMMON>, kRandThreads, 0) !=
            hipSuccess)
            o = 0;
        return (uint32_t)(o < 1 ? 1 : (o > 8 ? 8 : o));
    }();
    return v;
}

// One launch for any batch: a persistent word loop over as many blocks as are
// resident at once, one counter-sink unit per wave (at most 8,192 on 256 CUs).
hipError_t launch_rand(const RunArgs& a, uint32_t policy, uint32_t coin, uint32_t phases, uint8_t* decided) {
    if (a.n < 1 || a.n > (uint32_t)kMaxN || a.batch == 0 || phases < 1 || phases > kRandMaxPhases ||
        policy > 1 || coin > 1)
        return hipErrorInvalidValue;
    constexpr uint32_t wpb = kRandThreads / 64;
    const uint64_t words = (a.batch + 63) / 64;
    const bool gen = a.gen.faulty_mode != 0 || a.gen.order_mode != 0;
    ProfScope ps(a.prof, "k_rand", a.stream);
    auto go = [&](auto kernel, uint32_t per_cu) {
        uint64_t blocks = (words + wpb - 1) / wpb;
        const uint64_t cap = (uint64_t)per_cu * a.cu_count;  // persistent word loop beyond
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(kRandThreads), 0, a.stream, a.n, a.m,
                           phases, a.seed, a.gen, a.first_trial, a.batch, a.faulty, a.order,
                           a.decisions, a.outcome, decided, a.counters, a.sink);
    };
    auto pick = [&](auto coin_policy, auto common) {
        constexpr bool C = decltype(coin_policy)::value, M = decltype(common)::value;
        if (gen) go(k_rand<true, C, M>, rand_blocks_per_cu<true, C, M>());
        else go(k_rand<false, C, M>, rand_blocks_per_cu<false, C, M>());
    };
    if (policy == 0) {
        if (coin == 1) pick(std::true_type{}, std::true_type{});
        else pick(std::true_type{}, std::false_type{});
    } else {
        if (coin == 1) pick(std::false_type{}, std::true_type{});
        else pick(std::false_type{}, std::false_type{});
    }
    return hipGetLastError();
}

}  // namespace ba
