// ba_king.hip -- Phase King agreement (Berman, Garay, Perry; docs/SEMANTICS.md §9),
// one 64-trial word per wave (k_king, gfx950).
//
// Every general keeps one preference bit; bit-sliced over the word that is one
// plane per general (bit b = trial 64 w + b).  A phase is an exchange round, in
// which every general counts the attack votes it is shown by all n generals, and
// a king round.  Layout of a wave, for any n <= 32:
//   lane (i, s) = i + 32 s   recipient i < n, sender slice s: general i's preference
//                            plane, kept alike by both of its lanes
//   lane b                   trial b of the word for the inputs, `settled` and the epilogue
// Slice s takes the sender pairs u = s, s + 2, .. (senders 2u and 2u + 1): the
// work of an exchange round is 64 lanes wide for n = 32 and a lane walks at most
// eight pairs.  One Philox call yields the coins one sender shows recipients r and
// r ^ 1, so of a lane pair (i, i ^ 1) the even lane draws sender 2u's call, the
// odd lane sender 2u + 1's, and they swap the halves they do not need (one DPP
// quad_perm per 32-bit half): ceil(n/2) n calls per exchange round, ceil(n/2) per
// king round and for the commander's send (ba_king_coin_calls).
// Per wave, in LDS (3,096 B; four waves per block, no block barrier):
//   F[j]        faulty plane of general j (ballots over the trials' masks; 0 for j >= n)
//   pref[j]     what the senders hold this round (0 for j >= n); every lane of a
//               slice reads the same pref[j]: an LDS broadcast
//   part[p][l]  plane p of lane l's tally (up to 16 votes: five planes; lanes
//               consecutive: no bank conflict), read back by lane l ^ 32
//   kmaj, agr   the king's majority plane; the loyal attack / retreat holders of `settled`
// The DS instructions of one wave execute in issue order, so between the steps
// only the compiler has to be held (wave_sync, ba_wave_proto.hpp; the King
// helpers are ba_king_common.hpp's, shared with k_king3).
//
// Three wave-uniform shortcuts, all invisible in the results: a group of calls
// none of whose senders is faulty in a trial of the word is not drawn (a loyal
// sender's coin is never read), BA_KING_SPLIT draws nothing at all, and a king
// loyal throughout the word draws no king coins.
#include "ba_king_common.hpp"

namespace ba {

constexpr uint32_t kKingTag = 128;   // Philox ctr word 1 of round q: kKingTag + q
constexpr int kKingThreads = 256;    // four independent waves
constexpr int kKingPartPlanes = 5;   // a slice counts at most 16 votes

struct KingWave {
    uint64_t F[kMaxN];
    uint64_t pref[kMaxN];
    uint64_t part[kKingPartPlanes][64];
    uint64_t kmaj;
    uint64_t agr[2];
};

// One group of G sender pairs of an exchange round: this lane's pairs are
// u = v0 + 2 g + s.  Adds the 2 G votes general i is shown into its tally.
template <bool COIN, int G>
__device__ __forceinline__ void king_exchange_group(const KingWave& s, uint32_t i, uint32_t sl,
                                                    uint32_t v0, uint32_t n, uint32_t npairs,
                                                    uint32_t q, uint64_t gw, uint64_t seed,
                                                    uint64_t mypref, Count<kKingPartPlanes>& tally) {
    const uint32_t odd = i & 1u;
    // Before the draw only what decides it is loaded (the planes of the votes come
    // after it: held across the calls they cost 16 G registers).
    uint32_t ja[G];
    bool act[G], need = false;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const uint32_t u = v0 + 2u * (uint32_t)g + sl;  // <= 15: senders 2u, 2u + 1 <= 31
        act[g] = u < npairs;
        ja[g] = 2u * (act[g] ? u : 0u);
        // the lane's own call is sender ja + odd's; it serves recipients i and i ^ 1
        need |= act[g] && s.F[ja[g] + odd] != 0 && (i & ~1u) < n;
    }
    uint64_t ca[G], cb[G];  // what a faulty sender 2u / 2u + 1 shows recipient i
#pragma unroll
    for (int g = 0; g < G; ++g) ca[g] = cb[g] = odd ? ~0ull : 0ull;  // BA_KING_SPLIT: r & 1
    if constexpr (COIN) {
        if (__ballot(need) != 0) {
            const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
            P4 c[G];
#pragma unroll
            for (int g = 0; g < G; ++g)
                c[g] = P4{16u * (ja[g] + odd) + (i >> 1), kKingTag + q, (uint32_t)gw, (uint32_t)(gw >> 32)};
            if constexpr (G == 1) c[0] = philox10(c[0], k0, k1);
            else philox10_n<G>(c, k0, k1);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const KingCoin h = king_halves(c[g], odd);
                const uint64_t got = swap_neighbour(h.give);
                ca[g] = odd ? got : h.keep;
                cb[g] = odd ? h.keep : got;
            }
        }
    }
    // the group's 2 G <= 8 votes carry-saved in compile-time order, then the count's
    // four digits added to the tally once (a ripple per vote cost twice the adders)
    Csa<4> votes;
    static_for_h<0, G>([&](auto gi) {
        constexpr int g = gi();
        // an inactive pair sends nothing; a general counts its own true value
        const uint64_t Pa = s.pref[ja[g]], Pb = s.pref[ja[g] + 1], Fa = s.F[ja[g]], Fb = s.F[ja[g] + 1];
        uint64_t ma = ja[g] == i ? mypref : (Pa & ~Fa) | (Fa & ca[g]);
        uint64_t mb = ja[g] + 1 == i ? mypref : (Pb & ~Fb) | (Fb & cb[g]);
        if (!act[g]) ma = mb = 0;
        votes.template add<2 * g>(ma);
        votes.template add<2 * g + 1>(mb);
    });
    uint64_t digit[4];
    votes.template resolve<0, 2 * G, false>(digit, 0);
    uint64_t carry = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const uint64_t t = tally.c[p];
        tally.c[p] = xor3(t, digit[p], carry);
        carry = maj3(t, digit[p], carry);
    }
    tally.c[4] ^= carry;
    static_assert(kKingPartPlanes == 5, "a slice's tally: up to 16 votes");
}

template <bool GEN, bool COIN>
__global__ __launch_bounds__(kKingThreads) void k_king(uint32_t n, uint32_t m, uint32_t phases,
                                                       uint64_t seed, GenSpec gen,
                                                       uint64_t first_trial, uint64_t batch,
                                                       const uint32_t* __restrict__ faulty,
                                                       const uint8_t* __restrict__ order,
                                                       uint64_t* __restrict__ decisions,
                                                       uint8_t* __restrict__ outcome,
                                                       uint8_t* __restrict__ settled,
                                                       uint64_t* __restrict__ counters, Sink sk) {
    __shared__ KingWave lds[kKingThreads / 64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const uint32_t i = lane & 31u, sl = lane >> 5;
    KingWave& s = lds[wv];
    const uint32_t all = general_mask(n);
    const uint32_t npairs = (n + 1) / 2;
    // the update's two thresholds: c1 >= S -> attack, c1 <= n - S -> retreat, else the king
    const uint32_t S = (n + 2 * m) / 2 + 1, Tmaj = n / 2 + 1;
    const uint64_t words = (batch + 63) / 64;
    const uint32_t nwaves = gridDim.x * (kKingThreads / 64), gwave = blockIdx.x * (kKingThreads / 64) + wv;
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
            const uint64_t c = king_one_coin<COIN, kKingTag>(0, i, 0, gw, seed);
            if (i != 0) pref = (OB & ~F0) | (F0 & c);
        }
        if (i >= n) pref = 0;
        uint32_t st = 255;  // settled so far (lane = trial)
        if (settled && king_agree(s, lane, n, pref, myF)) st = 0;
        for (uint32_t p = 1; p <= phases; ++p) {
            wave_sync();
            if (lane < 32) s.pref[lane] = pref;
            wave_sync();
            // exchange round q = 2p - 1
            Count<kKingPartPlanes> tally;
            for (uint32_t v0 = 0; v0 < npairs; v0 += 8) {
                const uint32_t left = npairs - v0;  // pairs of both slices: groups of ceil(left / 2)
                if (left > 6)
                    king_exchange_group<COIN, 4>(s, i, sl, v0, n, npairs, 2 * p - 1, gw, seed, pref, tally);
                else if (left > 4)
                    king_exchange_group<COIN, 3>(s, i, sl, v0, n, npairs, 2 * p - 1, gw, seed, pref, tally);
                else if (left > 2)
                    king_exchange_group<COIN, 2>(s, i, sl, v0, n, npairs, 2 * p - 1, gw, seed, pref, tally);
                else
                    king_exchange_group<COIN, 1>(s, i, sl, v0, n, npairs, 2 * p - 1, gw, seed, pref, tally);
            }
            // merge the two slices' tallies: c1 of general i, six planes
#pragma unroll
            for (int b = 0; b < kKingPartPlanes; ++b) s.part[b][lane] = tally.c[b];
            wave_sync();
            Count<kKingPartPlanes + 1> c1;
            {
                uint64_t carry = 0;
#pragma unroll
                for (int b = 0; b < kKingPartPlanes; ++b) {
                    const uint64_t o = s.part[b][lane ^ 32u];
                    c1.c[b] = xor3(tally.c[b], o, carry);
                    carry = maj3(tally.c[b], o, carry);
                }
                c1.c[kKingPartPlanes] = carry;
            }
            const uint64_t hi = c1.ge(S), lo = S <= n ? ~c1.ge(n - S + 1) : 0ull;
            // king round q = 2p: general k = p - 1 shows its majority
            const uint32_t k = p - 1;
            if (lane == k) s.kmaj = c1.ge(Tmaj);
            wave_sync();
            const uint64_t kmaj = s.kmaj, Fk = s.F[k];
            uint64_t km = kmaj;
            if (__ballot(Fk != 0) != 0) {
                const uint64_t c = king_one_coin<COIN, kKingTag>(k, i, 2 * p, gw, seed);
                if (i != k) km = (kmaj & ~Fk) | (Fk & c);
            }
            pref = hi | (~lo & km);
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
        uint32_t A = 0;
        for (uint32_t r = 1; r < n; ++r) A |= lane_bit(&s.pref[r], lane) << r;
        TrialResult res = trial_result(n, 0, fm, oc, A, 0);
        // in-bound is Phase King's: |F| <= m and n > 4m
        res.out = (res.out & ~32u) | ((res.nf <= m && n > 4 * m) ? 32u : 0u);
        if (live) {
            if (decisions) decisions[t] = res.dec;
            if (outcome) outcome[t] = (uint8_t)res.out;
            if (settled) settled[t] = (uint8_t)st;
        }
        lane_counts_add<false>(live, res, lane, mine);
    }
    sink_counters(lane, mine, gwave, nwaves, counters, sk);
}

// Resident blocks per CU of one instantiation (its registers decide: the coin
// kernels hold four interleaved Philox calls), asked of the runtime once.
template <bool GEN, bool COIN>
static uint32_t king_blocks_per_cu() {
    static const uint32_t v = [] {
        int o = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, k_king<GEN, COIN>, kKingThreads, 0) != hipSuccess)
            o = 0;
        return (uint32_t)(o < 1 ? 1 : (o > 8 ? 8 : o));
    }();
    return v;
}

// One launch for any batch: a persistent word loop over as many blocks as are
// resident at once, one counter-sink unit per wave (at most 8,192 on 256 CUs: 128
// per replica, far below the sink's 2^16).
hipError_t launch_king(const RunArgs& a, uint32_t policy, uint32_t phases, uint8_t* settled) {
    if (a.n < 1 || a.n > (uint32_t)kMaxN || a.batch == 0 || phases < 1 || phases > a.n || policy > 1)
        return hipErrorInvalidValue;
    constexpr uint32_t wpb = kKingThreads / 64;
    const uint64_t words = (a.batch + 63) / 64;
    const bool gen = a.gen.faulty_mode != 0 || a.gen.order_mode != 0;
    ProfScope ps(a.prof, "k_king", a.stream);
    auto go = [&](auto kernel, uint32_t per_cu) {
        uint64_t blocks = (words + wpb - 1) / wpb;
        const uint64_t cap = (uint64_t)per_cu * a.cu_count;  // persistent word loop beyond
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(kKingThreads), 0, a.stream, a.n, a.m,
                           phases, a.seed, a.gen, a.first_trial, a.batch, a.faulty, a.order,
                           a.decisions, a.outcome, settled, a.counters, a.sink);
    };
    if (policy == 0) {
        if (gen) go(k_king<true, true>, king_blocks_per_cu<true, true>());
        else go(k_king<false, true>, king_blocks_per_cu<false, true>());
    } else {
        if (gen) go(k_king<true, false>, king_blocks_per_cu<true, false>());
        else go(k_king<false, false>, king_blocks_per_cu<false, false>());
    }
    return hipGetLastError();
}

}  // namespace ba
