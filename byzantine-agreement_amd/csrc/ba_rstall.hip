// ba_rstall.hip -- RAND (Ben-Or phases, docs/SEMANTICS.md §13) against the stalling
// adversary of §15, one lane per trial, one 64-trial word per wave (k_rstall, gfx950).
//
// The traitors' messages are a closed form of the loyal state, so there is no walk over
// sender pairs and no message coin: a trial's generals are bits of 32-bit masks x, D, V
// in the lane's registers, and a phase is arithmetic on three classes of generals,
// each of which counts alike:
//   loyal           c1 = a + t, a = popc(x & ~fm), t = min(max(n/2 - a, 0), f); they
//                   propose alike, P1 or P0 is n - f or 0, the traitors answer with the
//                   other value (attack on a tie), so d1 and d0 follow
//   faulty, x = 1   c1 = a + 1 (the other traitors show it retreat), its own proposal
//   faulty, x = 0   c1 = a      beside the loyal ones; a traitor shows it none
// Each class gets v, the strong threshold and "no v" as one bit, spread over its mask.
// Only the toss calls Philox: BA_RAND_COMMON one call for the word, bit `lane` of it;
// BA_RAND_LOCAL lane g draws general g's word c(3p, 33 g), the words go through LDS
// (256 B per wave, no block barrier) and trial b picks bit b of each.  The wave ORs the
// trials' "no v" masks first: a general's word is drawn and picked only where some
// trial of the word tosses it, and a phase in which nobody tosses calls nothing.
//
// Early finish, invisible in the results: when every trial of the word is in bound
// (|F| <= m, n > 3m) and all n generals of each, the faulty ones' honest state
// included, have D set, every x equals the one decided value and stays there (§15),
// so the word's remaining phases are skipped.  A word with one out-of-bound trial runs
// all its phases.
#include "ba_king_common.hpp"

namespace ba {

constexpr uint32_t kRstallTag = 256;   // RAND's: Philox ctr word 1 of the toss of phase p is 256 + 3p
constexpr int kRstallThreads = 256;    // four independent waves

struct RstallWave {
    uint64_t toss[kMaxN];  // general g's 64-trial toss word of the phase
};

// x ORed over the wave's 64 lanes (uniform result): DPP within each 16-lane row, then
// the four rows by readlane, as wave_sum_u32 adds
__device__ __forceinline__ uint32_t wave_or_u32(uint32_t x) {
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, true);   // quad_perm [1,0,3,2]
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, true);   // quad_perm [2,3,0,1]
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xF, 0xF, true);  // row_half_mirror
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x140, 0xF, 0xF, true);  // row_mirror
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 0) | (uint32_t)__builtin_amdgcn_readlane((int)x, 16) |
           (uint32_t)__builtin_amdgcn_readlane((int)x, 32) | (uint32_t)__builtin_amdgcn_readlane((int)x, 48);
}

// All ones where a >= b, for counts well below 2^31: a subtraction and a shift in a vector
// register, where a comparison holds a lane mask in a scalar register pair.  A phase has a
// dozen of these alive at once, and the kernel is short of scalar registers as it is.
__device__ __forceinline__ uint32_t ge_mask(uint32_t a, uint32_t b) {
    return (uint32_t)((int32_t)(b - 1u - a) >> 31);
}

// What one class of generals, shown d1 attack and d0 retreat proposals, does: masks over
// the class `cls` of those set to attack, of those without a v, of those that pass the
// strong threshold, and of those that pass it with attack.
struct StallClass {
    uint32_t one, none, strong, strong1;
};
__device__ __forceinline__ StallClass stall_class(uint32_t cls, uint32_t d1, uint32_t d0, uint32_t T,
                                                  uint32_t Tm) {
    const uint32_t v0 = ge_mask(d0, Tm), v1 = ~v0 & ge_mask(d1, Tm);
    const uint32_t s0 = v0 & ge_mask(d0, T), s1 = v1 & ge_mask(d1, T);
    return StallClass{v1 & cls, ~(v0 | v1) & cls, (s0 | s1) & cls, s1 & cls};
}

template <bool GEN, bool COMMON>
__global__ __launch_bounds__(kRstallThreads) void k_rstall(uint32_t n, uint32_t m, uint32_t phases,
                                                           uint64_t seed, GenSpec gen,
                                                           uint64_t first_trial, uint64_t batch,
                                                           const uint32_t* __restrict__ faulty,
                                                           const uint8_t* __restrict__ order,
                                                           uint64_t* __restrict__ decisions,
                                                           uint8_t* __restrict__ outcome,
                                                           uint8_t* __restrict__ decided,
                                                           uint64_t* __restrict__ counters, Sink sk) {
    __shared__ RstallWave lds[kRstallThreads / 64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    RstallWave& s = lds[wv];
    const uint32_t all = general_mask(n);
    // 2c > n + m  <=>  c >= T (beyond n nobody proposes); d > m  <=>  d >= Tm
    const uint32_t T = (n + m) / 2 + 1, Tm = m + 1, half = n / 2;
    const uint64_t words = (batch + 63) / 64;
    const uint32_t nwaves = gridDim.x * (kRstallThreads / 64), gwave = blockIdx.x * (kRstallThreads / 64) + wv;
    uint64_t mine = 0;
    for (uint64_t w = gwave; w < words; w += nwaves) {
        const uint64_t t = w * 64 + lane, gw = (first_trial >> 6) + w;
        const bool live = t < batch;
        uint32_t fm, oc;
        trial_inputs<GEN>(live, n, all, seed, gen, first_trial, t, faulty, order, fm, oc);
        const uint32_t ob = oc == 1, loyal = all & ~fm;
        const uint32_t f = (uint32_t)__popc(fm), nl = n - f;
        // every trial of the word in bound (a trial past the batch has nobody faulty)
        const bool inb_all = n > 3 * m && __ballot(f > m) == 0;
        // round 0: a faulty commander shows a loyal lieutenant r the bit r & 1, a faulty
        // one retreat, and keeps its own order
        uint32_t x = (fm & 1u) ? ((0xAAAAAAAAu & loyal) | ob) : (ob ? all : 0u);
        uint32_t D = 0, V = 0;
        uint32_t st = 255;  // decided so far
        for (uint32_t p = 1; p <= phases; ++p) {
            // report: t traitors show the loyal generals attack
            const uint32_t a = (uint32_t)__popc(x & loyal);
            const uint32_t want = half > a ? half - a : 0u, tt = want < f ? want : f;
            const uint32_t cl = a + tt;
            // the loyal generals' proposal (never both), as the n - f proposals shown
            const uint32_t l1 = ge_mask(cl, T) & nl, l0 = ge_mask(n - cl, T) & nl;
            // propose: the traitors show the loyal generals retreat if P1 > P0, else attack
            const uint32_t f0 = ge_mask(l1, 1) & f, f1 = f - f0;
            const StallClass cL = stall_class(loyal, l1 + f1, l0 + f0, T, Tm);
            // a faulty general counts the loyal messages and its own true ones (nobody
            // is in its class where a + 1 > n: then f = 0)
            const StallClass c1 =
                stall_class(fm & x, l1 + (ge_mask(a + 1, T) & 1u), l0 + (ge_mask(n - (a + 1), T) & 1u), T, Tm);
            const StallClass c0 =
                stall_class(fm & ~x, l1 + (ge_mask(a, T) & 1u), l0 + (ge_mask(n - a, T) & 1u), T, Tm);
            const uint32_t none = cL.none | c1.none | c0.none;
            const uint32_t fresh = (cL.strong | c1.strong | c0.strong) & ~D;
            V |= fresh & (cL.strong1 | c1.strong1 | c0.strong1);
            D |= fresh;
            // toss: only where v does not exist
            uint32_t coin = 0;
            if constexpr (COMMON) {
                if (__ballot(none != 0) != 0) {
                    const uint64_t c = king_one_coin<true, kRstallTag>(0, 0, 3 * p, gw, seed);
                    coin = ((c >> lane) & 1ull) ? all : 0u;
                }
            } else {
                const uint32_t drawn = wave_or_u32(none);  // the generals some trial tosses
                if (drawn != 0) {
                    uint64_t c = 0;
                    if (lane < 32 && ((drawn >> lane) & 1u))
                        c = king_one_coin<true, kRstallTag>(lane, lane, 3 * p, gw, seed);
                    wave_sync();  // the previous phase has read toss
                    if (lane < 32) s.toss[lane] = c;
                    wave_sync();
                    for (uint32_t rest = drawn; rest != 0; rest &= rest - 1) {
                        const uint32_t g = (uint32_t)__builtin_ctz(rest);
                        coin |= lane_bit(&s.toss[g], lane) << g;
                    }
                }
            }
            x = cL.one | c1.one | c0.one | (none & coin);
            // end of the phase: `decided` and the early finish
            if (decided) {
                const uint32_t LD = loyal & D, a1 = LD & V, a0 = LD & ~V;
                // two decided values; a decided general moved; a loyal commander's order not kept
                const bool bad = (a1 != 0 && a0 != 0) || (LD & (x ^ V)) != 0 ||
                                 ((fm & 1u) == 0 && (ob ? a0 : a1) != 0);
                if (bad) st = 254;
                else if (st == 255 && (loyal & ~D) == 0) st = p;
            }
            if (inb_all && __ballot((all & ~D) != 0) == 0) break;  // early finish
        }
        // epilogue: decisions, quorum, flags
        TrialResult res = trial_result(n, 0, fm, oc, x, 0);
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

// Resident blocks per CU of one instantiation, asked of the runtime once.
template <bool GEN, bool COMMON>
static uint32_t rstall_blocks_per_cu() {
    static const uint32_t v = [] {
        int o = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&o, k_rstall<GEN, COMMON>, kRstallThreads, 0) !=
            hipSuccess)
            o = 0;
        return (uint32_t)(o < 1 ? 1 : (o > 8 ? 8 : o));
    }();
    return v;
}

// One launch for any batch: a persistent word loop over as many blocks as are
// resident at once, one counter-sink unit per wave (at most 8,192 on 256 CUs).
hipError_t launch_rstall(const RunArgs& a, uint32_t coin, uint32_t phases, uint8_t* decided) {
    if (a.n < 1 || a.n > (uint32_t)kMaxN || a.batch == 0 || phases < 1 || phases > kRstallMaxPhases ||
        coin > 1)
        return hipErrorInvalidValue;
    constexpr uint32_t wpb = kRstallThreads / 64;
    const uint64_t words = (a.batch + 63) / 64;
    const bool gen = a.gen.faulty_mode != 0 || a.gen.order_mode != 0;
    ProfScope ps(a.prof, "k_rstall", a.stream);
    auto go = [&](auto kernel, uint32_t per_cu) {
        uint64_t blocks = (words + wpb - 1) / wpb;
        const uint64_t cap = (uint64_t)per_cu * a.cu_count;  // persistent word loop beyond
        if (blocks > cap) blocks = cap;
        hipLaunchKernelGGL(kernel, dim3((uint32_t)blocks), dim3(kRstallThreads), 0, a.stream, a.n, a.m,
                           phases, a.seed, a.gen, a.first_trial, a.batch, a.faulty, a.order,
                           a.decisions, a.outcome, decided, a.counters, a.sink);
    };
    if (coin == 1) {
        if (gen) go(k_rstall<true, true>, rstall_blocks_per_cu<true, true>());
        else go(k_rstall<false, true>, rstall_blocks_per_cu<false, true>());
    } else {
        if (gen) go(k_rstall<true, false>, rstall_blocks_per_cu<true, false>());
        else go(k_rstall<false, false>, rstall_blocks_per_cu<false, false>());
    }
    return hipGetLastError();
}

}  // namespace ba
