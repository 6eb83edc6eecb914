// ba_kenum.hip -- Phase King and KING3 against EVERY traitor strategy of one case
// (docs/SEMANTICS.md §11): k_kenum (gfx950).  One case is (proto, n, m, faulty set
// F, order o); every message a traitor sends to a loyal general is a free bit (two
// in KING3's propose round), a strategy S is an assignment of the B free bits, and
// trial t of a call is strategy S = t.  The kernel draws nothing, loads no
// per-trial input and reads no table: there is nothing to upload.
//
// k_enum's stance (ba_enum.hip), not k_king's: one LANE holds one 64-strategy word
// w = S / 64 and the n preference planes of its generals in registers (N is a
// template parameter, so the plane arrays are never indexed dynamically); a wave
// takes a tile of 64 consecutive words.  F, o, m and the phase are wave-uniform,
// and with them the class of every message (truth / free / dead) and the index of
// its free bit,
//   base of the round + rank of the sender among the traitors * l
//                     + rank of the recipient among the loyal      (l = n - |F|),
// doubled in the propose round (lo, hi): SGPR arithmetic and scalar branches.
//
// A round's tally at recipient i splits into what every recipient sees alike, the
// loyal senders' true values, counted once per round (`ls`), and what only i sees:
//   i loyal    the |F| free planes addressed to it, by traitor rank
//   i faulty   its own true value; the other traitors' messages are dead
//              (retreat / no proposal) and add nothing
// So the sender's identity never matters below, only its rank, and a recipient's
// update needs nobody else's plane of the same round: preferences are updated in
// place.  What the king of the phase shows (its majority / its x) is worked out
// first, for the one general k = p - 1, with k's plane picked by uniform selects.
//
// All 12 counters come from planes, per lane = word, as in k_enum; the witness is
// the wave's lowest violating S, one 64-bit atomic min per wave that found one.
// The lane = trial pick-out of decisions / outcome bytes runs only when asked for,
// on one-wave blocks that keep the tile's decision planes in LDS.
#include "ba_enum_common.hpp"

#include <utility>

namespace ba {

constexpr int kKenumThreads = 256;
constexpr uint32_t kKenumBlocksPerCu = 8;

using KCount = Count<5>;  // a tally of at most 16 messages

// The case (uniform over the launch) and the lane's word.
struct KenumWord {
    uint32_t F, nf, ell;  // the faulty mask, |F|, the loyal generals
    uint32_t m;
    uint32_t wlo, whi;  // this lane's word index w = S / 64
};

// rank of general i among the loyal ones
__device__ __forceinline__ uint32_t kenum_lrank(const KenumWord& c, uint32_t i) {
    return (uint32_t)__popc(~c.F & ((1u << i) - 1u));
}

// `ls` plus what recipient i alone is shown in a one-bit round whose free bits
// start at `base`: mine = i's own true value (i faulty), rl = i's loyal rank
__device__ __forceinline__ KCount kenum_votes(const KenumWord& c, const KCount& ls, bool fi,
                                              uint64_t mine, uint32_t base, uint32_t rl) {
    KCount t = ls;
    if (fi) {
        t.add(mine);
    } else {
        for (uint32_t rf = 0; rf < c.nf; ++rf) t.add(enum_plane(base + rf * c.ell + rl, c.wlo, c.whi));
    }
    return t;
}

// KING3's proposal of a general that counted c1 attack votes: R = [c1 <= m],
// A = [c1 >= n - m] and not R (retreat wins when both hold)
template <int N>
__device__ __forceinline__ void king3_proposal(const KenumWord& c, const KCount& c1, uint64_t& A,
                                               uint64_t& R) {
    const uint32_t Tq = (uint32_t)N > c.m ? (uint32_t)N - c.m : 0u;
    R = ~c1.ge(c.m + 1u);
    A = c1.ge(Tq) & ~R;
}

// KING3's propose round at recipient i: x and sure.  lsA / lsR: the loyal senders'
// proposals; ownA / ownR: i's own (i faulty); pbase: the round's first free bit.
template <int N>
__device__ __forceinline__ void king3_propose(const KenumWord& c, const KCount& lsA, const KCount& lsR,
                                              bool fi, uint64_t ownA, uint64_t ownR, uint64_t pref,
                                              uint32_t pbase, uint32_t rl, uint64_t& x, uint64_t& sure) {
    KCount d1 = lsA, d0 = lsR;
    if (fi) {
        d1.add(ownA);
        d0.add(ownR);
    } else {
        for (uint32_t rf = 0; rf < c.nf; ++rf) {
            const uint32_t b = pbase + 2u * (rf * c.ell + rl);
            const uint64_t lo = enum_plane(b, c.wlo, c.whi), hi = enum_plane(b + 1u, c.wlo, c.whi);
            d1.add(lo & hi);   // lo = 1: the proposal is hi
            d0.add(lo & ~hi);  // lo = 0: no proposal, whatever hi is
        }
    }
    const uint32_t Tq = (uint32_t)N > c.m ? (uint32_t)N - c.m : 0u, Tm = c.m + 1u;
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
__device__ __forceinline__ void kenum_king_phase(const KenumWord& c, uint64_t (&pref)[N], uint32_t k,
                                                 uint32_t& base) {
    const uint32_t S = ((uint32_t)N + 2u * c.m) / 2u + 1u, Tmaj = (uint32_t)N / 2u + 1u;
    const uint32_t xbase = base, kbase = base + c.nf * c.ell;
    const bool Fk = ((c.F >> k) & 1u) != 0;
    KCount ls;
#pragma unroll
    for (int j = 0; j < N; ++j)
        if (!((c.F >> j) & 1u)) ls.add(pref[j]);
    // the king's own majority
    const uint64_t kmaj = kenum_votes(c, ls, Fk, kenum_pick<N>(pref, k), xbase, kenum_lrank(c, k)).ge(Tmaj);
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const bool fi = ((c.F >> i) & 1u) != 0;
        const uint32_t rl = kenum_lrank(c, (uint32_t)i);
        const KCount c1 = kenum_votes(c, ls, fi, pref[i], xbase, rl);
        const uint64_t hi = c1.ge(S), lo = S <= (uint32_t)N ? ~c1.ge((uint32_t)N - S + 1u) : 0ull;
        uint64_t km = kmaj;  // i = k, or a loyal king
        if (Fk && k != (uint32_t)i) km = fi ? 0ull : enum_plane(kbase + rl, c.wlo, c.whi);
        pref[i] = hi | (~lo & km);
    }
    base = kbase + (Fk ? c.ell : 0u);
}

// One KING3 phase (§10) over the word, king k.
template <int N>
__device__ __forceinline__ void kenum_king3_phase(const KenumWord& c, uint64_t (&pref)[N], uint32_t k,
                                                  uint32_t& base) {
    const uint32_t vbase = base, pbase = vbase + c.nf * c.ell, kbase = pbase + 2u * c.nf * c.ell;
    const bool Fk = ((c.F >> k) & 1u) != 0;
    KCount lsV;
#pragma unroll
    for (int j = 0; j < N; ++j)
        if (!((c.F >> j) & 1u)) lsV.add(pref[j]);
    // value round: the loyal generals' proposals, counted once (a faulty general's
    // own proposal is worked out again where it is counted, in its propose round)
    KCount lsA, lsR;
#pragma unroll
    for (int j = 0; j < N; ++j) {
        if (!((c.F >> j) & 1u)) {
            uint64_t A, R;
            king3_proposal<N>(c, kenum_votes(c, lsV, false, 0, vbase, kenum_lrank(c, (uint32_t)j)), A, R);
            lsA.add(A);
            lsR.add(R);
        }
    }
    // the king's x
    uint64_t kx, ksure;
    {
        const uint64_t pk = kenum_pick<N>(pref, k);
        uint64_t A = 0, R = 0;
        if (Fk) king3_proposal<N>(c, kenum_votes(c, lsV, true, pk, vbase, 0), A, R);
        king3_propose<N>(c, lsA, lsR, Fk, A, R, pk, pbase, kenum_lrank(c, k), kx, ksure);
    }
#pragma unroll
    for (int i = 0; i < N; ++i) {
        const bool fi = ((c.F >> i) & 1u) != 0;
        const uint32_t rl = kenum_lrank(c, (uint32_t)i);
        uint64_t A = 0, R = 0;
        if (fi) king3_proposal<N>(c, kenum_votes(c, lsV, true, pref[i], vbase, 0), A, R);
        uint64_t x, sure;
        king3_propose<N>(c, lsA, lsR, fi, A, R, pref[i], pbase, rl, x, sure);
        uint64_t km = kx;  // i = k (then km = x), or a loyal king
        if (Fk && k != (uint32_t)i) km = fi ? 0ull : enum_plane(kbase + rl, c.wlo, c.whi);
        pref[i] = (sure & x) | (~sure & km);
    }
    base = kbase + (Fk ? c.ell : 0u);
}

template <int PROTO, int N>
__global__ __launch_bounds__(kKenumThreads) void k_kenum(KenumCase g, uint64_t first_trial,
                                                         uint64_t batch,
                                                         uint64_t* __restrict__ decisions,
                                                         uint8_t* __restrict__ outcome,
                                                         uint64_t* __restrict__ counters,
                                                         unsigned long long* __restrict__ witness,
                                                         Sink sk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char kenum_lds[];
    constexpr uint32_t n = (uint32_t)N, L = n - 1u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wpb = blockDim.x >> 6;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const bool want_out = decisions != nullptr || outcome != nullptr;  // then wpb == 1 (launch_kenum)
    uint64_t* const dec = reinterpret_cast<uint64_t*>(kenum_lds);      // [L][64], want_out only

    KenumWord c;
    c.F = g.fmask;
    c.nf = (uint32_t)__popc(g.fmask);
    c.ell = n - c.nf;
    c.m = g.m;
    const bool F0 = (g.fmask & 1u) != 0;
    const uint32_t oc = g.order;
    const uint64_t ob = oc == 1u ? ~0ull : 0ull;
    // quorum thresholds (§2.4): every general answers, total = n
    uint32_t needed = 2u * ((n - 1u) / 3u) + 1u;
    if (n <= 3u) needed = n - 1u;
    if (n == 1u) needed = 1u;
    const uint32_t needA = needed - (oc == 1u ? 1u : 0u);                        // attack iff nA >= needA
    const int32_t maxN = (int32_t)(L + (oc == 0u ? 1u : 0u)) - (int32_t)needed;  // retreat iff nA <= maxN
    const bool inb = c.nf <= g.m && n > (PROTO == 0 ? 4u : 3u) * g.m;

    const uint64_t words = (batch + 63u) / 64u, tiles = (words + 63u) / 64u;
    const uint64_t w0 = first_trial >> 6;
    const uint32_t nwaves = gridDim.x * wpb, gwave = blockIdx.x * wpb + wv;
    // per-lane totals: trials, agreement, validity, quorum r / a / u, violations, attack
    uint64_t tT = 0, tAg = 0, tVa = 0, tQr = 0, tQa = 0, tQu = 0, tVi = 0, tAt = 0;
    uint64_t wit = ~0ull;
    for (uint64_t t = gwave; t < tiles; t += nwaves) {
        const uint64_t lw = t * 64u + lane;  // the lane's word of this call
        const uint64_t gw = w0 + lw;
        uint64_t lm = 0;                     // the word's strategies inside the call
        if (lw < words) {
            const uint64_t rem = batch - lw * 64u;
            lm = rem >= 64u ? ~0ull : ((1ull << rem) - 1ull);
        }
        c.wlo = (uint32_t)gw;
        c.whi = (uint32_t)(gw >> 32);
        // round 0: the commander sends
        uint64_t pref[N];
        pref[0] = ob;
#pragma unroll
        for (int i = 1; i < N; ++i) {
            if (!F0) pref[i] = ob;
            else if ((c.F >> i) & 1u) pref[i] = 0;  // dead
            else pref[i] = enum_plane(kenum_lrank(c, (uint32_t)i), c.wlo, c.whi);
        }
        uint32_t base = F0 ? c.ell : 0u;
        for (uint32_t p = 1; p <= g.phases; ++p) {
            if constexpr (PROTO == 0) kenum_king_phase<N>(c, pref, p - 1u, base);
            else kenum_king3_phase<N>(c, pref, p - 1u, base);
        }
        // decisions = the lieutenants' preferences; never undefined
        uint64_t allA = ~0ull, allR = ~0ull;
        KCount cA;
        uint32_t sumA = 0;
#pragma unroll
        for (int r = 1; r < N; ++r) {
            const uint64_t A = pref[r];
            if (!((c.F >> r) & 1u)) {  // a loyal lieutenant
                allA &= A;
                allR &= ~A;
            }
            cA.add(A);
            sumA += (uint32_t)__popcll(A & lm);
            if (want_out) dec[(uint32_t)(r - 1) * 64u + lane] = A;
        }
        const uint64_t agree = allA | allR;
        const uint64_t valid = F0 ? 0ull : (oc == 1u ? allA : allR);
        const uint64_t qr = maxN < 0 ? 0ull : ~cA.ge((uint32_t)maxN + 1u);
        const uint64_t qa = ~qr & cA.ge(needA);
        const uint64_t viol = lm & ~(agree & (F0 ? ~0ull : valid));
        tT += (uint32_t)__popcll(lm);
        tAg += (uint32_t)__popcll(agree & lm);
        tVa += (uint32_t)__popcll(valid & lm);
        tQr += (uint32_t)__popcll(qr & lm);
        tQa += (uint32_t)__popcll(qa & lm);
        tQu += (uint32_t)__popcll(~qr & ~qa & lm);
        tAt += sumA;
        tVi += (uint32_t)__popcll(viol);
        if (viol) {
            const uint64_t s = (gw << 6) + (uint64_t)__builtin_ctzll(viol);
            wit = s < wit ? s : wit;
        }
        if (want_out) {
            // lane = trial: the tile's words one by one out of the decision planes
            __syncthreads();  // one-wave blocks: the planes are written
            const uint32_t half = lane >> 5, sh = lane & 31u;
            for (uint32_t q = 0; q < 64u; ++q) {
                const uint64_t qw = t * 64u + q;
                if (qw >= words) break;
                const uint64_t i = qw * 64u + lane;
                uint32_t A = 0;
                for (uint32_t rr = 0; rr < L; ++rr) {
                    const uint32_t* d = reinterpret_cast<const uint32_t*>(dec + rr * 64u + q);
                    A |= ((d[half] >> sh) & 1u) << rr;
                }
                TrialResult res = trial_result(n, 0, g.fmask, oc, A << 1, 0);
                res.out = (res.out & ~32u) | (inb ? 32u : 0u);  // in-bound is the protocol's
                if (i < batch) {
                    if (decisions) decisions[i] = res.dec;
                    if (outcome) outcome[i] = (uint8_t)res.out;
                }
            }
            __syncthreads();  // the next tile rewrites the planes
        }
    }
    // wave totals: lane c holds counter c
    const uint64_t T = enum_wave_sum(tT), Ag = enum_wave_sum(tAg), Va = enum_wave_sum(tVa);
    const uint64_t Qr = enum_wave_sum(tQr), Qa = enum_wave_sum(tQa), Qu = enum_wave_sum(tQu);
    const uint64_t Vi = enum_wave_sum(tVi), At = enum_wave_sum(tAt);
    uint64_t tot[C_NUM];
    tot[C_TRIALS] = T;
    tot[C_AGREE] = Ag;
    tot[C_VAPPL] = F0 ? 0ull : T;  // F, and with it in-bound and the faulty count, is the call's
    tot[C_VALID] = Va;
    tot[C_QR] = Qr;
    tot[C_QA] = Qa;
    tot[C_QU] = Qu;
    tot[C_UNDEF] = 0;
    tot[C_INB] = inb ? T : 0ull;
    tot[C_VIOL] = inb ? Vi : 0ull;
    tot[C_FTOT] = (uint64_t)c.nf * T;
    tot[C_ATT] = At;
    uint64_t mine = 0;
#pragma unroll
    for (int i = 0; i < C_NUM; ++i)
        if (lane == (uint32_t)i) mine = tot[i];
    sink_counters(lane, mine, gwave, nwaves, counters, sk);
    if (witness) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint64_t o = __shfl_xor(wit, off, 64);
            wit = o < wit ? o : wit;
        }
        if (lane == 0 && wit != ~0ull) (void)atomicMin(witness, (unsigned long long)wit);
    }
}

using KenumKernel = void (*)(KenumCase, uint64_t, uint64_t, uint64_t*, uint8_t*, uint64_t*,
                             unsigned long long*, Sink);

template <int PROTO, size_t... I>
static KenumKernel kenum_kernel_of(uint32_t n, std::index_sequence<I...>) {
    static constexpr KenumKernel tab[] = {k_kenum<PROTO, (int)I + 1>...};
    return tab[n - 1u];
}

// One persistent launch: a wave per tile of 64 words (4,096 strategies), at most
// kKenumBlocksPerCu four-wave blocks per CU; one counter-sink unit per wave.  With
// per-trial outputs the blocks are one wave each and hold (n - 1) x 64 decision
// planes in LDS (at most 7.5 KiB).
hipError_t launch_kenum(const RunArgs& a, const KenumCase& g, uint64_t* witness) {
    if (a.n < 1 || a.n > kKenumMaxN || g.proto > 1 || a.batch == 0 || g.phases < 1 || g.phases > a.n)
        return hipErrorInvalidValue;
    const bool want_out = a.decisions != nullptr || a.outcome != nullptr;
    const uint32_t threads = want_out ? 64u : (uint32_t)kKenumThreads, wpb = threads / 64u;
    const uint32_t lds = want_out ? (a.n - 1u) * 64u * (uint32_t)sizeof(uint64_t) : 0u;
    const uint64_t words = (a.batch + 63) / 64, tiles = (words + 63) / 64;
    uint64_t blocks = (tiles + wpb - 1) / wpb;
    const uint64_t cap = (uint64_t)kKenumBlocksPerCu * a.cu_count * (kKenumThreads / threads);
    if (blocks > cap) blocks = cap;
    ProfScope ps(a.prof, "k_kenum", a.stream);
    const KenumKernel k = g.proto == 0 ? kenum_kernel_of<0>(a.n, std::make_index_sequence<kKenumMaxN>{})
                                       : kenum_kernel_of<1>(a.n, std::make_index_sequence<kKenumMaxN>{});
    hipLaunchKernelGGL(k, dim3((uint32_t)blocks), dim3(threads), lds, a.stream, g, a.first_trial, a.batch,
                       a.decisions, a.outcome, a.counters, (unsigned long long*)witness, a.sink);
    return hipGetLastError();
}

}  // namespace ba
