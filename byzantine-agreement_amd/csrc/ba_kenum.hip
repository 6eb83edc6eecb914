// ba_kenum.hip -- Phase King and KING3 against EVERY traitor strategy of one case
// (docs/SEMANTICS.md §11): k_kenum (gfx950).  One case is (proto, n, m, faulty set
// F, order o); every message a traitor sends to a loyal general is a free bit (two
// in KING3's propose round), a strategy S is an assignment of the B free bits, and
// trial t of a call is strategy S = t.  The kernel draws nothing, loads no
// per-trial input and reads no table: there is nothing to upload.
//
// The lane = word stance, the numbering of the free bits and the split of a round's
// tally into the loyal senders' sum and the recipient's own view are
// ba_round_enum.hpp's; the planes here are the n preferences.  What the king of the
// phase shows (its majority / its x) is worked out first, for the one general
// k = p - 1, with k's plane picked by uniform selects.
//
// The tile loop, the counters, the witness and the per-trial outputs are the frame
// of ba_enum_common.hpp; the word evaluator below hands it the lieutenants' planes.
#include "ba_round_enum.hpp"

namespace ba {

// KING3's proposal of a general that counted c1 attack votes: R = [c1 <= m],
// A = [c1 >= n - m] and not R (retreat wins when both hold)
template <int N>
__device__ __forceinline__ void king3_proposal(uint32_t m, const RoundCount& c1, uint64_t& A, uint64_t& R) {
    const uint32_t Tq = (uint32_t)N > m ? (uint32_t)N - m : 0u;
    R = ~c1.ge(m + 1u);
    A = c1.ge(Tq) & ~R;
}

// KING3's propose round at recipient i: x and sure.  lsA / lsR: the loyal senders'
// proposals; ownA / ownR: i's own (i faulty); pbase: the round's first free bit.
template <int N>
__device__ __forceinline__ void king3_propose(const RoundWord& c, uint32_t m, const RoundCount& lsA,
                                              const RoundCount& lsR, bool fi, uint64_t ownA, uint64_t ownR,
                                              uint64_t pref, uint32_t pbase, uint32_t rl, uint64_t& x,
                                              uint64_t& sure) {
    RoundCount d1 = lsA, d0 = lsR;
    if (fi) {
        d1.add(ownA);
        d0.add(ownR);
    } else {
        round_proposals(c, d1, d0, pbase, rl);
    }
    const uint32_t Tq = (uint32_t)N > m ? (uint32_t)N - m : 0u, Tm = m + 1u;
    const uint64_t x0 = d0.ge(Tm), x1 = d1.ge(Tm);
    x = ~x0 & (x1 | pref);
    sure = (x & d1.ge(Tq)) | (~x & d0.ge(Tq));
}

// the plane of general k (uniform) out of the register array
template <int N>
__device__ __forceinline__ uint64_t kenum_pick(const uint64_t (&pref)[N], uint32_t k) {
    uint64_t v = 0;
#pragma unroll
    for (int i = 0; i < N; ++i)
        if (k == (uint32_t)i) v = pref[i];
    return v;
}

// One Phase King phase (§9) over the word, king k; base: the exchange round's
// first free bit, advanced past the phase.
template <int N>
__device__ __forceinline__ void kenum_king_phase(const RoundWord& c, uint32_t m, uint64_t (&pref)[N],
                                                 uint32_t k, uint32_t& base) {
    const uint32_t S = ((uint32_t)N + 2u * m) / 2u + 1u, Tmaj = (uint32_t)N / 2u + 1u;
    const uint32_t xbase = base, kbase = base + c.nf * c.ell;
    const bool Fk = ((c.F >> k) & 1u) != 0;
    const RoundCount ls = round_loyal(c, pref);
    // the king's own majority
    const uint64_t kmaj = round_votes(c, ls, Fk, kenum_pick<N>(pref, k), xbase, round_lrank(c, k)).ge(Tmaj);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const bool fi = ((c.F >> i) & 1u) != 0;
        const uint32_t rl = round_lrank(c, (uint32_t)i);
        const RoundCount c1 = round_votes(c, ls, fi, pref[i], xbase, rl);
        const uint64_t hi = c1.ge(S), lo = S <= (uint32_t)N ? ~c1.ge((uint32_t)N - S + 1u) : 0ull;
        uint64_t km = kmaj;  // i = k, or a loyal king
        if (Fk && k != (uint32_t)i) km = fi ? 0ull : enum_plane(kbase + rl, c.wlo, c.whi);
        pref[i] = hi | (~lo & km);
    }
    base = kbase + (Fk ? c.ell : 0u);
}

// One KING3 phase (§10) over the word, king k.
template <int N>
__device__ __forceinline__ void kenum_king3_phase(const RoundWord& c, uint32_t m, uint64_t (&pref)[N],
                                                  uint32_t k, uint32_t& base) {
    const uint32_t vbase = base, pbase = vbase + c.nf * c.ell, kbase = pbase + 2u * c.nf * c.ell;
    const bool Fk = ((c.F >> k) & 1u) != 0;
    const RoundCount lsV = round_loyal(c, pref);
    // value round: the loyal generals' proposals, counted once (a faulty general's
    // own proposal is worked out again where it is counted, in its propose round)
    RoundCount lsA, lsR;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if (!((c.F >> j) & 1u)) {
            uint64_t A, R;
            king3_proposal<N>(m, round_votes(c, lsV, false, 0, vbase, round_lrank(c, (uint32_t)j)), A, R);
            lsA.add(A);
            lsR.add(R);
        }
    }
    // the king's x
    uint64_t kx, ksure;
    {
        const uint64_t pk = kenum_pick<N>(pref, k);
        uint64_t A = 0, R = 0;
        if (Fk) king3_proposal<N>(m, round_votes(c, lsV, true, pk, vbase, 0), A, R);
        king3_propose<N>(c, m, lsA, lsR, Fk, A, R, pk, pbase, round_lrank(c, k), kx, ksure);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const bool fi = ((c.F >> i) & 1u) != 0;
        const uint32_t rl = round_lrank(c, (uint32_t)i);
        uint64_t A = 0, R = 0;
        if (fi) king3_proposal<N>(m, round_votes(c, lsV, true, pref[i], vbase, 0), A, R);
        uint64_t x, sure;
        king3_propose<N>(c, m, lsA, lsR, fi, A, R, pref[i], pbase, rl, x, sure);
        uint64_t km = kx;  // i = k (then km = x), or a loyal king
        if (Fk && k != (uint32_t)i) km = fi ? 0ull : enum_plane(kbase + rl, c.wlo, c.whi);
        pref[i] = (sure & x) | (~sure & km);
    }
    base = kbase + (Fk ? c.ell : 0u);
}

template <int PROTO, int N>
__global__ __launch_bounds__(kEnumThreads) void k_kenum(KenumCase g, uint64_t first_trial,
                                                        uint64_t batch,
                                                        uint64_t* __restrict__ decisions,
                                                        uint8_t* __restrict__ outcome,
                                                        uint64_t* __restrict__ counters,
                                                        unsigned long long* __restrict__ witness,
                                                        Sink sk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char kenum_lds[];
    constexpr uint32_t n = (uint32_t)N;
    const bool F0 = (g.fmask & 1u) != 0;
    const uint64_t ob = g.order == 1u ? ~0ull : 0ull;
    // in-bound is the protocol's
    const bool inb = (uint32_t)__popc(g.fmask) <= g.m && n > (PROTO == 0 ? 4u : 3u) * g.m;
    const EnumRun run{n, g.fmask, g.order, 0u, inb, first_trial, batch, decisions, outcome, counters, witness};
    enum_frame<false, true>(run, kenum_lds, sk, [&](uint32_t wlo, uint32_t whi, EnumTally<false>& ty) {
        const RoundWord c = round_word(g.fmask, n, wlo, whi);
        // round 0: the commander sends (spelled out here and in k_renum: as a shared
        // helper it cost k_kenum<0, 2> two VGPRs and with them a wave per SIMD)
        uint64_t pref[N];
        pref[0] = ob;
#pragma unroll
        for (int i = 1; i < N; ++i) {
            if (!F0) pref[i] = ob;
            else if ((c.F >> i) & 1u) pref[i] = 0;  // dead
            else pref[i] = enum_plane(round_lrank(c, (uint32_t)i), c.wlo, c.whi);
        }
        uint32_t base = F0 ? c.ell : 0u;
        for (uint32_t p = 1; p <= g.phases; ++p) {
            if constexpr (PROTO == 0) kenum_king_phase<N>(c, g.m, pref, p - 1u, base);
            else kenum_king3_phase<N>(c, g.m, pref, p - 1u, base);
        }
        round_decide(c, pref, ty);
    });
}

using KenumKernel = void (*)(KenumCase, uint64_t, uint64_t, uint64_t*, uint8_t*, uint64_t*,
                             unsigned long long*, Sink);

// One persistent launch of enum_geometry's shape (at most 7.5 KiB of decision planes).
hipError_t launch_kenum(const RunArgs& a, const KenumCase& g, uint64_t* witness) {
    if (a.n < 1 || a.n > kKenumMaxN || g.proto > 1 || a.batch == 0 || g.phases < 1 || g.phases > a.n)
        return hipErrorInvalidValue;
    const EnumGeometry ge = enum_geometry(a, (uint32_t)sizeof(EnumEntry<false>), 0u);
    ProfScope ps(a.prof, "k_kenum", a.stream);
    const KenumKernel k = round_kernel_of<kKenumMaxN>(a.n, [&](auto N) -> KenumKernel {
        return g.proto == 0 ? k_kenum<0, decltype(N)::value> : k_kenum<1, decltype(N)::value>;
    });
    hipLaunchKernelGGL(k, dim3(ge.blocks), dim3(ge.threads), ge.lds, a.stream, g, a.first_trial, a.batch,
                       a.decisions, a.outcome, a.counters, (unsigned long long*)witness, a.sink);
    return hipGetLastError();
}

}  // namespace ba
