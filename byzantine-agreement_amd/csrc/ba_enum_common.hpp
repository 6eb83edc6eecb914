// ba_enum_common.hpp -- what the four exhaustive kernels share: k_enum (ba_enum.hip,
// docs/SEMANTICS.md §8), k_kenum (ba_kenum.hip, §11), k_smenum (ba_smenum.hip, §12)
// and k_renum (ba_renum.hip, §14); what only the round-based two of them share is
// ba_round_enum.hpp.  Trial t of a call is strategy S = t; one lane holds one
// 64-strategy word w = S / 64, a free bit of the strategy index is a plane of it
// (enum_plane), and a wave takes a tile of 64 consecutive words.
//
// enum_frame is everything around the evaluation of one word: the persistent tile
// loop, the word's mask of strategies inside the call, the tally of the lieutenants'
// decision planes into the 12 counters (per lane = word, reduced once per wave at the
// end, through sink_counters), the witness (the wave's lowest violating S, one 64-bit
// atomic min per wave that found one) and, only when asked for, the lane = trial
// pick-out of decisions / outcome bytes, on one-wave blocks that keep the tile's
// decision planes in LDS.  A kernel is its case set-up and a word evaluator
// word(wlo, whi, tally), which hands every lieutenant's decision plane to
// tally.put().  enum_geometry is the launch shape that goes with the frame.
#pragma once
#include "ba_wave_proto.hpp"

namespace ba {

constexpr int kEnumThreads = 256;
constexpr uint32_t kEnumBlocksPerCu = 8;

// plane of free bit i (uniform) in word w
__device__ __forceinline__ uint64_t enum_plane(uint32_t i, uint32_t wlo, uint32_t whi) {
    if (i < 6u) {
        return i == 0u   ? 0xAAAAAAAAAAAAAAAAull
               : i == 1u ? 0xCCCCCCCCCCCCCCCCull
               : i == 2u ? 0xF0F0F0F0F0F0F0F0ull
               : i == 3u ? 0xFF00FF00FF00FF00ull
               : i == 4u ? 0xFFFF0000FFFF0000ull
                         : 0xFFFFFFFF00000000ull;
    }
    const uint32_t sh = i - 6u;
    const uint32_t h = sh < 32u ? wlo : whi;
    const int32_t s = (int32_t)(h << (31u - (sh & 31u))) >> 31;  // -(bit sh of w)
    return (uint64_t)(int64_t)s;
}

__device__ __forceinline__ uint64_t enum_wave_sum(uint64_t x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, 64);
    return x;
}

// x becomes the wave's smallest.  In place: taken and returned by value, the same
// loop cost k_kenum and k_renum two VGPRs each, and two of them a wave per SIMD.
__device__ __forceinline__ void enum_wave_min(uint64_t& x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const uint64_t o = __shfl_xor(x, off, 64);
        x = o < x ? o : x;
    }
}

// One launch of a case, as the frame sees it.  me and inb: OM(m)'s depth for
// trial_result (0 elsewhere) and whether the case is within the protocol's bound.
struct EnumRun {
    uint32_t n, fmask, order, me;
    bool inb;
    uint64_t first_trial, batch;
    uint64_t* decisions;
    uint8_t* outcome;
    uint64_t* counters;
    unsigned long long* witness;
};

// A decision-plane entry in LDS: attack, and with UNDEF (OM(m)) undefined beside it.
template <bool UNDEF>
struct __attribute__((aligned(UNDEF ? 16 : 8))) EnumEntry {
    uint64_t p[UNDEF ? 2 : 1];
};

// The tally of one word.  put(r, loyal, A[, U]): lieutenant rank r (general r + 1)
// decides attack on plane A, is undefined on U, retreats elsewhere.
template <bool UNDEF>
struct EnumTally {
    uint64_t lm;                  // the word's strategies inside the call
    EnumEntry<UNDEF>* dec;        // LDS [n - 1][64], this lane's column; want_out only
    bool want_out;
    uint64_t allA = ~0ull, allU = ~0ull, allR = ~0ull;  // over the loyal lieutenants
    Count<5> cA, cN;              // attack decisions; attack or undefined ones
    uint32_t sumA = 0, sumU = 0;

    __device__ __forceinline__ void put(uint32_t r, bool loyal, uint64_t A, uint64_t U = 0ull) {
        if (loyal) {
            allA &= A;
            if constexpr (UNDEF) allU &= U;
            allR &= ~(A | U);
        }
        cA.add(A);
        sumA += (uint32_t)__popcll(A & lm);
        if constexpr (UNDEF) {
            cN.add(A | U);
            sumU += (uint32_t)__popcll(U & lm);
            if (want_out) dec[r * 64u] = EnumEntry<true>{{A, U}};
        } else {
            if (want_out) dec[r * 64u] = EnumEntry<false>{{A}};
        }
    }

    // The lieutenants of rank mask rs, none of them loyal, all decide A (SM(m)'s
    // traitors share one V): their attack sum is one popcount.
    __device__ __forceinline__ void put_same(uint32_t rs, uint64_t A) {
        static_assert(!UNDEF, "one plane per lieutenant");
        sumA += (uint32_t)__popc(rs) * (uint32_t)__popcll(A & lm);
        for (; rs; rs &= rs - 1u) {
            cA.add(A);
            if (want_out) dec[(uint32_t)__builtin_ctz(rs) * 64u] = EnumEntry<false>{{A}};
        }
    }
};

// UNDEF: decisions may be undefined (OM(m)): the second plane, its counter and the
// 16-byte entries.  OWN_INB: outcome bit 5 is g.inb, the protocol's own bound, not
// trial_result's (OM(m)'s n > 3m).  plane_lds: (n - 1) x 64 entries, used with
// per-trial outputs only; then the blocks are one wave each (enum_geometry).
template <bool UNDEF, bool OWN_INB, typename Word>
__device__ __forceinline__ void enum_frame(const EnumRun& g, unsigned char* plane_lds, const Sink& sk,
                                           Word&& word) {
    const uint32_t n = g.n, L = n - 1u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wpb = blockDim.x >> 6;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const bool want_out = g.decisions != nullptr || g.outcome != nullptr;
    EnumEntry<UNDEF>* const dec = reinterpret_cast<EnumEntry<UNDEF>*>(plane_lds);
    const bool F0 = (g.fmask & 1u) != 0;
    const uint32_t oc = g.order;
    // quorum thresholds (§2.4): every general answers, total = n
    uint32_t needed = 2u * ((n - 1u) / 3u) + 1u;
    if (n <= 3u) needed = n - 1u;
    if (n == 1u) needed = 1u;
    const uint32_t needA = needed - (oc == 1u ? 1u : 0u);                        // attack iff nA >= needA
    const int32_t maxN = (int32_t)(L + (oc == 0u ? 1u : 0u)) - (int32_t)needed;  // retreat iff nA + nU <= maxN
    const uint32_t nf = (uint32_t)__popc(g.fmask);

    const uint64_t batch = g.batch;
    const uint64_t words = (batch + 63u) / 64u, tiles = (words + 63u) / 64u;
    const uint64_t w0 = g.first_trial >> 6;
    const uint32_t nwaves = gridDim.x * wpb, gwave = blockIdx.x * wpb + wv;
    // per-lane totals: trials, agreement, validity, quorum r / a / u, undefined, violations, attack
    uint64_t tT = 0, tAg = 0, tVa = 0, tQr = 0, tQa = 0, tQu = 0, tUn = 0, tVi = 0, tAt = 0;
    uint64_t wit = ~0ull;
    for (uint64_t t = gwave; t < tiles; t += nwaves) {
        const uint64_t lw = t * 64u + lane;  // the lane's word of this call
        const uint64_t gw = w0 + lw;
        EnumTally<UNDEF> ty;
        ty.lm = 0;
        if (lw < words) {
            const uint64_t rem = batch - lw * 64u;
            ty.lm = rem >= 64u ? ~0ull : ((1ull << rem) - 1ull);
        }
        ty.dec = dec + lane;
        ty.want_out = want_out;
        word((uint32_t)gw, (uint32_t)(gw >> 32), ty);
        const uint64_t lm = ty.lm;
        const uint64_t agree = UNDEF ? (ty.allA | ty.allU | ty.allR) : (ty.allA | ty.allR);
        const uint64_t valid = F0 ? 0ull : (oc == 1u ? ty.allA : ty.allR);
        const uint64_t qr = maxN < 0 ? 0ull : ~(UNDEF ? ty.cN : ty.cA).ge((uint32_t)maxN + 1u);
        const uint64_t qa = ~qr & ty.cA.ge(needA);
        const uint64_t viol = lm & ~(agree & (F0 ? ~0ull : valid));
        tT += (uint32_t)__popcll(lm);
        tAg += (uint32_t)__popcll(agree & lm);
        tVa += (uint32_t)__popcll(valid & lm);
        tQr += (uint32_t)__popcll(qr & lm);
        tQa += (uint32_t)__popcll(qa & lm);
        tQu += (uint32_t)__popcll(~qr & ~qa & lm);
        if constexpr (UNDEF) tUn += ty.sumU;
        tAt += ty.sumA;
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
                uint32_t A = 0, U = 0;
                for (uint32_t rr = 0; rr < L; ++rr) {
                    const uint32_t* d = reinterpret_cast<const uint32_t*>(dec + rr * 64u + q);
                    A |= ((d[half] >> sh) & 1u) << rr;
                    if constexpr (UNDEF) U |= ((d[2u + half] >> sh) & 1u) << rr;
                }
                TrialResult res = trial_result(n, g.me, g.fmask, oc, A << 1, U << 1);
                if constexpr (OWN_INB) res.out = (res.out & ~32u) | (g.inb ? 32u : 0u);
                if (i < batch) {
                    if (g.decisions) g.decisions[i] = res.dec;
                    if (g.outcome) g.outcome[i] = (uint8_t)res.out;
                }
            }
            __syncthreads();  // the next tile rewrites the planes
        }
    }
    // wave totals: lane c holds counter c
    const uint64_t T = enum_wave_sum(tT), Ag = enum_wave_sum(tAg), Va = enum_wave_sum(tVa);
    const uint64_t Qr = enum_wave_sum(tQr), Qa = enum_wave_sum(tQa), Qu = enum_wave_sum(tQu);
    const uint64_t Un = UNDEF ? enum_wave_sum(tUn) : 0ull;
    const uint64_t Vi = enum_wave_sum(tVi), At = enum_wave_sum(tAt);
    uint64_t tot[C_NUM];
    tot[C_TRIALS] = T;
    tot[C_AGREE] = Ag;
    tot[C_VAPPL] = F0 ? 0ull : T;  // F, and with it in-bound and the faulty count, is the call's
    tot[C_VALID] = Va;
    tot[C_QR] = Qr;
    tot[C_QA] = Qa;
    tot[C_QU] = Qu;
    tot[C_UNDEF] = Un;
    tot[C_INB] = g.inb ? T : 0ull;
    tot[C_VIOL] = g.inb ? Vi : 0ull;
    tot[C_FTOT] = (uint64_t)nf * T;
    tot[C_ATT] = At;
    uint64_t mine = 0;
#pragma unroll
    for (int i = 0; i < C_NUM; ++i)
        if (lane == (uint32_t)i) mine = tot[i];
    sink_counters(lane, mine, gwave, nwaves, g.counters, sk);
    if (g.witness) {
        enum_wave_min(wit);
        if (lane == 0 && wit != ~0ull) (void)atomicMin(g.witness, (unsigned long long)wit);
    }
}

// The launch shape of an enumeration kernel: a wave per tile of 64 words (4,096
// strategies), at most kEnumBlocksPerCu four-wave blocks per CU; one counter-sink
// unit per wave.  With per-trial outputs the blocks are one wave each and hold
// (n - 1) x 64 decision-plane entries of entry_bytes in LDS, after lds_before
// bytes of the kernel's own (k_enum's slot map).
struct EnumGeometry {
    uint32_t blocks, threads, lds;
};

inline EnumGeometry enum_geometry(const RunArgs& a, uint32_t entry_bytes, uint32_t lds_before) {
    const bool want_out = a.decisions != nullptr || a.outcome != nullptr;
    const uint32_t threads = want_out ? 64u : (uint32_t)kEnumThreads, wpb = threads / 64u;
    const uint32_t lds = lds_before + (want_out ? (a.n - 1u) * 64u * entry_bytes : 0u);
    const uint64_t words = (a.batch + 63) / 64, tiles = (words + 63) / 64;
    uint64_t blocks = (tiles + wpb - 1) / wpb;
    const uint64_t cap = (uint64_t)kEnumBlocksPerCu * a.cu_count * (kEnumThreads / threads);
    if (blocks > cap) blocks = cap;
    return {(uint32_t)blocks, threads, lds};
}

}  // namespace ba
