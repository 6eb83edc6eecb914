// ba_king3.hip -- the three-round King algorithm (Berman, Garay, Perry;
// docs/SEMANTICS.md §10), one 64-trial word per wave (k_king3, gfx950).
//
// k_king's layout (ba_king.hip) carries over: one preference plane per general,
// lane (i, s) = i + 32 s is recipient i < n with sender slice s (pairs u = s,
// s + 2, ..: senders 2u and 2u + 1), lane b is trial b for the inputs, `settled`
// and the epilogue; one Philox call yields what one sender shows recipients r and
// r ^ 1, swapped between the lanes of a pair by DPP; tallies are carry-saved per
// group of sender pairs and merged across the two slices through wave-private LDS.
// A phase has three rounds:
//   value    c1 = the attack votes shown; proposals A = [c1 >= n - m] and
//            R = [c1 <= m] (retreat wins when both hold)
//   propose  every sender shows one of (attack, retreat, nothing): two sender
//            planes A[j], R[j] in LDS, disjoint for a loyal j; a faulty j shows
//            the coin as A and its complement as R.  One walk over the sender
//            pairs feeds two tallies d1 and d0; x = 0 if d0 > m, 1 if d1 > m,
//            else pref; sure = [d_x >= n - m]
//   king     general k = p - 1 shows x_k to those who are not sure
// Per wave, in LDS (3,608 B; four waves per block, no block barrier):
//   F[j], pref[j]   as in k_king
//   pa[j], pr[j]    the proposal planes of the propose round (0 for j >= n)
//   part[p][l]      plane p of lane l's tally, read back by lane l ^ 32; the two
//                   tallies of the propose round pass through it one after the other
//   kx, agr         the king's x plane; the loyal attack / retreat holders of `settled`
// The King helpers are ba_king_common.hpp's, shared with k_king; so is the walk
// over the sender pairs of the value and propose rounds (king3_round, king3_merge),
// which k_rand takes too.  The wave helpers are ba_wave_proto.hpp's.
//
// The three wave-uniform shortcuts of k_king hold here too, invisible in the
// results: a group of calls none of whose senders is faulty in a trial of the
// word is not drawn, BA_KING_SPLIT draws nothing, and a king loyal throughout
// the word draws no king coins.
#include "ba_king_common.hpp"

namespace ba {

constexpr uint32_t kKing3Tag = 192;   // Philox ctr word 1 of round q: kKing3Tag + q
constexpr int kKing3Threads = 256;    // four independent waves

struct King3Wave {
    uint64_t F[kMaxN];
    uint64_t pref[kMaxN];
    uint64_t pa[kMaxN], pr[kMaxN];
    uint64_t part[kKing3PartPlanes][64];
    uint64_t kx;
    uint64_t agr[2];
};

template <bool GEN, bool COIN>
__global__ __launch_bounds__(kKing3Threads) void k_king3(uint32_t n, uint32_t m, uint32_t phases,
                                                         uint64_t seed, GenSpec gen,
                                                         uint64_t first_trial, uint64_t batch,
                                                         const uint32_t* __restrict__ faulty,
                                                         const uint8_t* __restrict__ order,
                                                         uint64_t* __restrict__ decisions,
                                                         uint8_t* __restrict__ outcome,
                                                         uint8_t* __restrict__ settled,
                                                         uint64_t* __restrict__ counters, Sink sk) {
    __shared__ King3Wave lds[kKing3Threads / 64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t i = lane & 31u, sl = lane >> 5;
    King3Wave& s = lds[wv];
    const uint32_t all = general_mask(n);
    const uint32_t npairs = (n + 1) / 2;
    // the thresholds, compared as signed integers: n - m <= 0 always holds
    // (Count::ge(0) is all ones); m + 1 <= 11
    const uint32_t Tq = n > m ? n - m : 0u, Tm = m + 1;
    const uint64_t words = (batch + 63) / 64;
    const uint32_t nwaves = gridDim.x * (kKing3Threads / 64), gwave = blockIdx.x * (kKing3Threads / 64) + wv;
    uint64_t mine = 0;
    for (uint64_t w = gwave; w < words; w += nwaves) {
        const uint64_t t = w * 64 + lane, gw = (first_trial >> 6) + w;
        const bool live = t < batch;
        uint32_t fm, oc;
        trial_inputs<GEN>(live, n, all, seed, gen, first_trial, t, faulty, order, fm, oc);
        // planes of the word
        const uint64_t OB = __ballot(oc == 1);
        uint64_t myF = 0, F0 = 0;
        for (uint32_t g = 0; g < n; ++g) {
            const uint64_t pl = faulty_plane(fm, g);
            if (g == 0) F0 = pl;
            if (i == g) myF = pl;
        }
        wave_sync();  // the previous word's epilogue has read pref
        if (lane < 32) s.F[lane] = myF;
        // round 0: the commander sends
        uint64_t pref = OB;
        if (F0 != 0) {
            const uint64_t c = king_one_coin<COIN, kKing3Tag>(0, i, 0, gw, seed);
            if (i != 0) pref = (OB & ~F0) | (F0 & c);
        }
        if (i >= n) pref = 0;
        uint32_t st = 255;  // settled so far (lane = trial)
        if (settled && king_agree(s, lane, n, pref, myF)) st = 0;
        for (uint32_t p = 1; p <= phases; ++p) {
            wave_sync();
            if (lane < 32) s.pref[lane] = pref;
            wave_sync();
            // value round q = 3p - 2
            uint64_t A, R;
            {
                Tally3 tv, unused;
                king3_round<kKing3Tag, COIN, false>(s, i, sl, n, npairs, 3 * p - 2, gw, seed, pref, 0, tv, unused);
                const auto c1 = king3_merge(s, lane, tv);
                R = ~c1.ge(Tm);  // c0 >= n - m  <=>  c1 <= m
                A = c1.ge(Tq) & ~R;  // retreat wins when both hold (n <= 2m)
            }
            if (i >= n) A = R = 0;  // a general that is not there proposes nothing
            if (lane < 32) {
                s.pa[lane] = A;
                s.pr[lane] = R;
            }
            wave_sync();
            // propose round q = 3p - 1
            uint64_t x, sure;
            {
                Tally3 ta, tr;
                king3_round<kKing3Tag, COIN, true>(s, i, sl, n, npairs, 3 * p - 1, gw, seed, A, R, ta, tr);
                const auto d1 = king3_merge(s, lane, ta);
                const uint64_t x1 = d1.ge(Tm), s1 = d1.ge(Tq);
                const auto d0 = king3_merge(s, lane, tr);
                const uint64_t x0 = d0.ge(Tm), s0 = d0.ge(Tq);
                x = ~x0 & (x1 | pref);
                sure = (x & s1) | (~x & s0);
            }
            // king round q = 3p: general k = p - 1 shows its x
            const uint32_t k = p - 1;
            if (lane == k) s.kx = x;
            wave_sync();
            const uint64_t kx = s.kx, Fk = s.F[k];
            uint64_t km = kx;
            if (__ballot(Fk != 0) != 0) {
                const uint64_t c = king_one_coin<COIN, kKing3Tag>(k, i, 3 * p, gw, seed);
                if (i != k) km = (kx & ~Fk) | (Fk & c);
            }
            pref = (sure & x) | (~sure & km);  // i = k: km = x
            if (i >= n) pref = 0;
            if (settled) {
                const bool ag = king_agree(s, lane, n, pref, myF);
                st = ag ? (st == 255 ? p : st) : 255u;
            }
        }
        // epilogue, lane = trial: decisions, quorum, flags
        wave_sync();
        if (lane < 32) s.pref[lane] = pref;
        wave_sync();
        uint32_t Adec = 0;
        for (uint32_t r = 1; r < n; ++r) Adec |= lane_bit(&s.pref[r], lane) << r;
        TrialResult res = trial_result(n, 0, fm, oc, Adec, 0);
        // in-bound is this protocol's: |F| <= m and n > 3m
        res.out = (res.out & ~32u) | ((res.nf <= m && n > 3 * m) ? 32u : 0u);
        if (live) {
            if (decisions) decisions[t] = res.dec;
            if (outcome) outcome[t] = (uint8_t)res.out;
            if (settled) settled[t] = (uint8_t)st;
        }
        lane_counts_add<false>(live, res, lane, mine);
    }
    sink_counters(lane, mine, gwave, nwaves, counters, sk);
}

// Resident blocks per CU of one instantiation (its registers decide), asked of
// the runtime once.
template <bool GEN, bool COIN>
static uint32_t king3_blocks_per_cu() {
    static const uint32_t v = [] {
        int o = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, k_king3<GEN, COIN>, kKing3Threads, 0) != hipSuccess)
            o = 0;
        return (uint32_t)(o < 1 ? 1 : (o > 8 ? 8 : o));
    }();
    return v;
}

// One launch for any batch: a persistent word loop over as many blocks as are
// resident at once, one counter-sink unit per wave (at most 8,192 on 256 CUs).
hipError_t launch_king3(const RunArgs& a, uint32_t policy, uint32_t phases, uint8_t* settled) {
    if (a.n < 1 || a.n > (uint32_t)kMaxN || a.batch == 0 || phases < 1 || phases > a.n || policy > 1)
        return hipErrorInvalidValue;
    constexpr uint32_t wpb = kKing3Threads / 64;
    const uint64_t words = (a.batch + 63) / 64;
    const bool gen = a.gen.faulty_mode != 0 || a.gen.order_mode != 0;
    ProfScope ps(a.prof, "k_king3", a.stream);
    auto go = [&](auto kernel, uint32_t per_cu) {
        uint64_t blocks = (words + wpb - 1) / wpb;
        const uint64_t cap = (uint64_t)per_cu * a.cu_count;  // persistent word loop beyond
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(kKing3Threads), 0, a.stream, a.n, a.m,
                           phases, a.seed, a.gen, a.first_trial, a.batch, a.faulty, a.order,
                           a.decisions, a.outcome, settled, a.counters, a.sink);
    };
    if (policy == 0) {
        if (gen) go(k_king3<true, true>, king3_blocks_per_cu<true, true>());
        else go(k_king3<false, true>, king3_blocks_per_cu<false, true>());
    } else {
        if (gen) go(k_king3<true, false>, king3_blocks_per_cu<true, false>());
        else go(k_king3<false, false>, king3_blocks_per_cu<false, false>());
    }
    return hipGetLastError();
}

}  // namespace ba
