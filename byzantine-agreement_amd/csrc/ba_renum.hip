// ba_renum.hip -- RAND (Ben-Or phases, docs/SEMANTICS.md §13) against EVERY traitor
// strategy and EVERY coin outcome of one case (§14): k_renum (gfx950).  One case is
// (coin, n, m, R, faulty set F, order o); every message a traitor sends to a loyal
// general is a free bit (two for a proposal: lo = 0 withholds it), and so is every
// toss: one bit per loyal general and phase under BA_RAND_LOCAL, one bit per phase
// under BA_RAND_COMMON.  A strategy S is an assignment of the B free bits and trial t
// of a call is strategy S = t, so a walk of the space covers every play of every
// adversary, the one that sees the coins included.  Nothing is drawn or loaded.
//
// The lane = word stance, the numbering of a message's free bit and the split of a
// round's tally into the loyal senders' sum and the recipient's own view are
// ba_round_enum.hpp's; the planes here are x, D, V of the N generals, and a phase's
// toss bits follow its proposals: base + rl (LOCAL), base (COMMON).  A faulty
// general's D and V reach no output and stay zero.
//
// `decided` on planes: a sticky unsafe plane built from §13's three conditions at the
// end of every phase, a sticky all-loyal-decided plane, and the phase of the latter's
// first setting in five bit-planes.  The tile loop, the counters, the IC1/IC2 witness
// and the decisions / outcome pick-out are the frame of ba_enum_common.hpp; the stats
// are per-lane sums in what the word evaluator captures, reduced once per wave after
// the frame returns.
#include "ba_round_enum.hpp"

namespace ba {

// One phase (§13) over the word.  base: the report round's first free bit, advanced
// past the phase's toss bits.
template <bool COMMON, int N>
__device__ __forceinline__ void renum_phase(const RoundWord& c, uint32_t T, uint32_t Tm, uint64_t (&x)[N],
                                            uint64_t (&D)[N], uint64_t (&V)[N], uint32_t& base) {
    const uint32_t rbase = base, pbase = rbase + c.nf * c.ell, tbase = pbase + 2u * c.nf * c.ell;
    const uint32_t Tr = (uint32_t)N - T + 1u;  // c0 >= T  <=>  c1 <= n - T  <=>  not c1 >= Tr (T <= n)
    const RoundCount ls = round_loyal(c, x);
    // report: the loyal generals' proposals, counted once (a faulty general's own is
    // worked out where it is counted, in its propose round)
    RoundCount lsA, lsR;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if (!((c.F >> j) & 1u)) {
            const RoundCount c1 = round_votes(c, ls, false, 0, rbase, round_lrank(c, (uint32_t)j));
            lsA.add(c1.ge(T));
            lsR.add(T <= (uint32_t)N ? ~c1.ge(Tr) : 0ull);
        }
    }
    const uint64_t common = COMMON ? enum_plane(tbase, c.wlo, c.whi) : 0ull;
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const bool fi = ((c.F >> i) & 1u) != 0;
        const uint32_t rl = round_lrank(c, (uint32_t)i);
        RoundCount d1 = lsA, d0 = lsR;
        uint64_t coin = common;
        if (fi) {
            const RoundCount c1 = round_votes(c, ls, true, x[i], rbase, 0);
            d1.add(c1.ge(T));
            d0.add(T <= (uint32_t)N ? ~c1.ge(Tr) : 0ull);
        } else {
            round_proposals(c, d1, d0, pbase, rl);
            if (!COMMON) coin = enum_plane(tbase + rl, c.wlo, c.whi);
        }
        const uint64_t v0 = d0.ge(Tm), v1 = d1.ge(Tm) & ~v0;
        if (!fi) {
            const uint64_t fresh = ((v0 & d0.ge(T)) | (v1 & d1.ge(T))) & ~D[i];
            V[i] |= fresh & v1;
            D[i] |= fresh;
        }
        x[i] = v1 | (~(v0 | v1) & coin);
    }
    base = tbase + (COMMON ? 1u : c.ell);
}

template <bool COMMON, int N>
__global__ __launch_bounds__(kEnumThreads) void k_renum(RenumCase g, uint64_t first_trial, uint64_t batch,
                                                        uint64_t* __restrict__ decisions,
                                                        uint8_t* __restrict__ outcome,
                                                        uint8_t* __restrict__ decided,
                                                        uint64_t* __restrict__ counters,
                                                        unsigned long long* __restrict__ witness,
                                                        unsigned long long* __restrict__ stats, Sink sk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char renum_lds[];
    constexpr uint32_t n = (uint32_t)N;
    const bool F0 = (g.fmask & 1u) != 0;
    const uint64_t ob = g.order == 1u ? ~0ull : 0ull;
    const uint32_t T = (n + g.m) / 2u + 1u, Tm = g.m + 1u;
    const bool inb = (uint32_t)__popc(g.fmask) <= g.m && n > 3u * g.m;
    // per-lane stats: unsafe, undecided, their smallest S, decided in phase p
    uint32_t sUns = 0, sUnd = 0, sIn[kRenumMaxPhases];
#pragma unroll
    for (int p = 0; p < (int)kRenumMaxPhases; ++p) sIn[p] = 0;
    uint64_t wUns = ~0ull, wUnd = ~0ull;
    const EnumRun run{n, g.fmask, g.order, 0u, inb, first_trial, batch, decisions, outcome, counters, witness};
    enum_frame<false, true>(run, renum_lds, sk, [&](uint32_t wlo, uint32_t whi, EnumTally<false>& ty) {
        const RoundWord c = round_word(g.fmask, n, wlo, whi);
        // round 0: the commander sends (as in k_kenum, which says why it is spelled out)
        uint64_t x[N], D[N], V[N];
        x[0] = ob;
#pragma unroll
        for (int i = 1; i < N; ++i) {
            if (!F0) x[i] = ob;
            else if ((c.F >> i) & 1u) x[i] = 0;  // dead
            else x[i] = enum_plane(round_lrank(c, (uint32_t)i), c.wlo, c.whi);
        }
        uint32_t base = F0 ? c.ell : 0u;
#pragma unroll
        for (int i = 0; i < N; ++i) D[i] = V[i] = 0;
        uint64_t bad = 0, seen = 0, ph[5] = {0, 0, 0, 0, 0};
        for (uint32_t p = 1; p <= g.phases; ++p) {
            renum_phase<COMMON, N>(c, T, Tm, x, D, V, base);
            // the end of the phase over the loyal generals (a faulty one's D is clear)
            uint64_t a1 = 0, a0 = 0, moved = 0, allD = ~0ull;
#pragma unroll
            for (int i = 0; i < N; ++i) {
                a1 |= D[i] & V[i];
                a0 |= D[i] & ~V[i];
                moved |= D[i] & (x[i] ^ V[i]);
                if (!((c.F >> i) & 1u)) allD &= D[i];
            }
            // two decided values; a decided general moved; a loyal commander's order not kept
            bad |= (a1 & a0) | moved | (F0 ? 0ull : ((a1 & ~ob) | (a0 & ob)));
            const uint64_t first = allD & ~seen;
            seen |= allD;
#pragma unroll
            for (int b = 0; b < 5; ++b)
                if ((p >> b) & 1u) ph[b] |= first;
        }
        round_decide(c, x, ty);
        const uint64_t lm = ty.lm, gw = ((uint64_t)whi << 32) | wlo;
        const uint64_t uns = bad & lm, und = ~bad & ~seen & lm, in = ~bad & seen & lm;
        sUns += (uint32_t)__popcll(uns);
        sUnd += (uint32_t)__popcll(und);
        if (uns) {
            const uint64_t s = (gw << 6) + (uint64_t)__builtin_ctzll(uns);
            wUns = s < wUns ? s : wUns;
        }
        if (und) {
            const uint64_t s = (gw << 6) + (uint64_t)__builtin_ctzll(und);
            wUnd = s < wUnd ? s : wUnd;
        }
#pragma unroll
        for (int p = 1; p <= (int)kRenumMaxPhases; ++p) {
            if ((uint32_t)p <= g.phases) {
                uint64_t eq = in;
#pragma unroll
                for (int b = 0; b < 5; ++b) eq &= ((p >> b) & 1) ? ph[b] : ~ph[b];
                sIn[p - 1] += (uint32_t)__popcll(eq);
            }
        }
        if (decided) {
            // the word's bytes, written by its lane: tests and windows, not a hot path
            const uint64_t at = (gw << 6) - first_trial;
            for (uint32_t b = 0; b < 64u; ++b) {
                if (!((lm >> b) & 1ull)) continue;
                uint32_t v = 0;
#pragma unroll
                for (int k = 0; k < 5; ++k) v |= (uint32_t)((ph[k] >> b) & 1ull) << k;
                if (!((seen >> b) & 1ull)) v = 255u;
                if ((bad >> b) & 1ull) v = 254u;
                decided[at + b] = (uint8_t)v;
            }
        }
    });
    if (stats) {
        // wave totals: lane k holds stats[k]
        const uint32_t lane = threadIdx.x & 63u;
        uint64_t mine = 0;
        const uint64_t tUns = enum_wave_sum(sUns), tUnd = enum_wave_sum(sUnd);
        if (lane == 0) mine = tUns;
        if (lane == 1) mine = tUnd;
#pragma unroll
        for (int p = 0; p < (int)kRenumMaxPhases; ++p) {
            const uint64_t t = enum_wave_sum(sIn[p]);
            if (lane == (uint32_t)(4 + p)) mine = t;
        }
        enum_wave_min(wUns);
        enum_wave_min(wUnd);
        if (lane == 2 || lane == 3) {
            const uint64_t w = lane == 2 ? wUns : wUnd;
            if (w != ~0ull) (void)atomicMin(stats + lane, (unsigned long long)w);
        } else if (lane < kRenumStats && mine != 0) {
            (void)atomicAdd(stats + lane, (unsigned long long)mine);
        }
    }
}

using RenumKernel = void (*)(RenumCase, uint64_t, uint64_t, uint64_t*, uint8_t*, uint8_t*, uint64_t*,
                             unsigned long long*, unsigned long long*, Sink);

// One persistent launch of enum_geometry's shape (at most 7.5 KiB of decision planes).
hipError_t launch_renum(const RunArgs& a, const RenumCase& g, uint8_t* decided, uint64_t* witness,
                        uint64_t* stats) {
    if (a.n < 1 || a.n > kRenumMaxN || g.coin > 1 || a.batch == 0 || g.phases < 1 ||
        g.phases > kRenumMaxPhases)
        return hipErrorInvalidValue;
    const EnumGeometry ge = enum_geometry(a, (uint32_t)sizeof(EnumEntry<false>), 0u);
    ProfScope ps(a.prof, "k_renum", a.stream);
    const RenumKernel k = round_kernel_of<kRenumMaxN>(a.n, [&](auto N) -> RenumKernel {
        return g.coin == 1 ? k_renum<true, decltype(N)::value> : k_renum<false, decltype(N)::value>;
    });
    hipLaunchKernelGGL(k, dim3(ge.blocks), dim3(ge.threads), ge.lds, a.stream, g, a.first_trial, a.batch,
                       a.decisions, a.outcome, decided, a.counters, (unsigned long long*)witness,
                       (unsigned long long*)stats, a.sink);
    return hipGetLastError();
}

}  // namespace ba
