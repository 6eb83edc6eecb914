// ba_enum.hip -- OM(m) against EVERY traitor strategy of one case (docs/SEMANTICS.md
// §8): k_enum (gfx950).  One case is (n, m, faulty set F, order o); every message a
// traitor sends to a loyal lieutenant is a free bit, a strategy S is an assignment
// of the B free bits, and trial t of a call is strategy S = t.  The kernel draws
// nothing and loads no per-trial input.
//
// Bit-sliced: one 64-bit plane = one value for the 64 strategies of a word
// w = S / 64.  Free bit i < 6 is a constant plane (it varies inside the word), bit
// i >= 6 is bit i - 6 of w spread over the plane.  A work item is (word, receiver);
// the layout is receiver-major: a wave takes a tile of 64 consecutive words, one
// per lane, and walks the receivers r = 0..L-1 one after the other, so at any
// moment the wave holds 64 words of ONE receiver.  F, o and r are then
// wave-uniform, and with them the class of every slot (truth / free / dead), the
// slot's rank, its byte in the slot map and the i < 6 constants: they live in
// SGPRs and the branches on them are scalar.  Only the i >= 6 planes and the
// values derived from them differ per lane.
//
// The walk is k_adv's depth-first receiver walk (ba_adv.hip): lieutenant r's root
// decision over its relay chains sigma, carrying
//   x    the truth plane L_{k-1}[sigma]
//   Fs   whether sigma's last lieutenant (the sender below) is faulty: uniform
//   sr   the slot rank of sigma at level k-1; the rank of sigma j at level k is
//        sr (L - k) + popcount(lieutenants not in sigma that are below j)
// with children in rank order and the carry-save counters of adv_resolve.  A
// message of a loyal sender is x; one of a faulty sender is looked up by rank in
// the per-level byte map (LDS, built on the host): dead -> retreat, bit i -> its
// plane.
//
// All 12 counters come from planes, per lane = word: IC1 / IC2 by AND over the
// loyal receivers' {attack, undefined, retreat} planes, the quorum by three
// bit-sliced counters and ge(), the sums by popcount; per-lane totals are reduced
// once per wave at the end and go through sink_counters.  The witness is the
// wave's lowest violating S, one 64-bit atomic min per wave that found one.  The
// lane = trial pick-out of decisions / outcome bytes runs only when asked for, on
// one-wave blocks that keep the tile's decision planes in LDS.  enum_plane and
// enum_wave_sum are ba_enum_common.hpp's, shared with k_kenum.
#include "ba_enum_common.hpp"

namespace ba {

constexpr int kEnumThreads = 256;
constexpr uint32_t kEnumBlocksPerCu = 8;

struct __attribute__((aligned(16))) EnumPair {
    uint64_t a, u;  // attack, undefined
};

struct EnumWalk {
    const uint8_t* map;  // LDS: the slot map, level k at off[k]
    uint32_t off[kEnumLevels];
    uint32_t L, r, fl;   // fl: bit j = lieutenant rank j is faulty
    uint32_t wlo, whi;   // this lane's word index w = S / 64
};

// value of the slot `rank` of level K whose sender is faulty: free or dead
template <int K>
__device__ __forceinline__ uint64_t enum_slot(const EnumWalk& c, uint32_t rank) {
    const uint32_t code = (uint32_t)__builtin_amdgcn_readfirstlane((int)c.map[c.off[K] + rank]);
    if (code >= kEnumTruth) return 0ull;  // dead (a faulty sender's slot is never truth)
    return enum_plane(code, c.wlo, c.whi);
}

// resolve_r(sigma) of §2.3 for |sigma| = K under §8's lie rule.  notin: the
// lieutenants not in sigma (r among them); sr: sigma's slot rank at level K-1 (0 at
// the root).  tie (K == 0 only): the root's undefined plane.
template <int K, int ME>
__device__ __forceinline__ uint64_t enum_resolve(const EnumWalk& c, uint64_t x, bool Fs, uint32_t sr,
                                                 uint32_t notin, uint64_t& tie) {
    const uint32_t s = c.L - (uint32_t)K;  // popcount(notin): the node's inputs
    const uint32_t base = sr * s;
    const uint64_t val = Fs ? enum_slot<K>(c, base + __popc(notin & ((1u << c.r) - 1u))) : x;
    if constexpr (K == ME) {
        return val;
    } else {
        const uint32_t nch = s - 1u;
        Count<5> cnt;  // L - K <= 31 inputs
        cnt.c[0] = val;
        uint32_t it = notin & ~(1u << c.r);
        uint64_t pend = 0;
        for (uint32_t ch = 0; ch < nch; ++ch) {
            const uint32_t j = (uint32_t)__builtin_ctz(it);
            it &= it - 1u;
            const uint32_t rank = base + ch + (j > c.r ? 1u : 0u);
            const uint64_t xc = Fs ? enum_slot<K>(c, rank) : x;
            uint64_t dummy;
            const uint64_t e = enum_resolve<K + 1, ME>(c, xc, ((c.fl >> j) & 1u) != 0, rank,
                                                       notin ^ (1u << j), dummy);
            if (ch & 1u) {  // carry-save: two results and plane 0 through one full adder
                uint64_t carry = maj3(cnt.c[0], pend, e);
                cnt.c[0] = xor3(cnt.c[0], pend, e);
#pragma unroll
                for (int i = 1; i < 5; ++i) {
                    const uint64_t t = cnt.c[i] & carry;
                    cnt.c[i] ^= carry;
                    carry = t;
                }
            } else {
                pend = e;
            }
        }
        if (nch & 1u) cnt.add(pend);
        const uint64_t maj = cnt.ge(s / 2u + 1u);  // strict majority = more than s / 2
        if constexpr (K == 0) tie = (s & 1u) ? 0ull : (cnt.ge(s / 2u) & ~maj);
        return maj;
    }
}

template <int ME>
__global__ __launch_bounds__(kEnumThreads) void k_enum(EnumCase g, uint64_t first_trial,
                                                       uint64_t batch,
                                                       const uint8_t* __restrict__ map,
                                                       uint64_t* __restrict__ decisions,
                                                       uint8_t* __restrict__ outcome,
                                                       uint64_t* __restrict__ counters,
                                                       unsigned long long* __restrict__ witness,
                                                       Sink sk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char enum_lds[];
    const uint32_t n = g.n, L = n - 1u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wpb = blockDim.x >> 6;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const bool want_out = decisions != nullptr || outcome != nullptr;  // then wpb == 1 (launch_enum)
    // the slot map: g.map_bytes (a multiple of 16) bytes of the ctx's scratch -> LDS
    for (uint32_t i = tid * 4u; i < g.map_bytes; i += blockDim.x * 4u)
        *reinterpret_cast<uint32_t*>(enum_lds + i) = *reinterpret_cast<const uint32_t*>(map + i);
    EnumPair* const dec = reinterpret_cast<EnumPair*>(enum_lds + g.map_bytes);  // [L][64], want_out only
    __syncthreads();

    EnumWalk c;
    c.map = enum_lds;
#pragma unroll
    for (int k = 0; k < kEnumLevels; ++k) c.off[k] = g.off[k];
    c.L = L;
    c.fl = g.fmask >> 1;
    const bool F0 = (g.fmask & 1u) != 0;
    const uint32_t oc = g.order;
    const uint64_t ob = oc == 1u ? ~0ull : 0ull;
    const uint32_t lts = general_mask(L);
    // quorum thresholds (§2.4): every general answers, total = n
    uint32_t needed = 2u * ((n - 1u) / 3u) + 1u;
    if (n <= 3u) needed = n - 1u;
    if (n == 1u) needed = 1u;
    const uint32_t needA = needed - (oc == 1u ? 1u : 0u);          // attack iff nA >= needA
    const int32_t maxN = (int32_t)(L + (oc == 0u ? 1u : 0u)) - (int32_t)needed;  // retreat iff nA + nU <= maxN
    const uint32_t nf = __popc(g.fmask);
    const bool inb = nf <= (uint32_t)ME && n > 3u * (uint32_t)ME;

    const uint64_t words = (batch + 63u) / 64u, tiles = (words + 63u) / 64u;
    const uint64_t w0 = first_trial >> 6;
    const uint32_t nwaves = gridDim.x * wpb, gwave = blockIdx.x * wpb + wv;
    // per-lane totals: trials, agreement, validity, quorum r / a / u, undefined, violations, attack
    uint64_t tT = 0, tAg = 0, tVa = 0, tQr = 0, tQa = 0, tQu = 0, tUn = 0, tVi = 0, tAt = 0;
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
        uint64_t allA = ~0ull, allU = ~0ull, allR = ~0ull;
        Count<5> cA, cN;  // attack decisions; attack or undefined ones
        uint32_t sumA = 0, sumU = 0;
        for (uint32_t r = 0; r < L; ++r) {
            c.r = r;
            uint64_t U = 0;
            const uint64_t A = enum_resolve<0, ME>(c, ob, F0, 0u, lts, U);
            if (!((c.fl >> r) & 1u)) {  // a loyal lieutenant
                allA &= A;
                allU &= U;
                allR &= ~(A | U);
            }
            cA.add(A);
            cN.add(A | U);
            sumA += (uint32_t)__popcll(A & lm);
            sumU += (uint32_t)__popcll(U & lm);
            if (want_out) dec[r * 64u + lane] = EnumPair{A, U};
        }
        const uint64_t agree = allA | allU | allR;
        const uint64_t valid = F0 ? 0ull : (oc == 1u ? allA : allR);
        const uint64_t qr = maxN < 0 ? 0ull : ~cN.ge((uint32_t)maxN + 1u);
        const uint64_t qa = ~qr & cA.ge(needA);
        const uint64_t viol = lm & ~(agree & (F0 ? ~0ull : valid));
        tT += (uint32_t)__popcll(lm);
        tAg += (uint32_t)__popcll(agree & lm);
        tVa += (uint32_t)__popcll(valid & lm);
        tQr += (uint32_t)__popcll(qr & lm);
        tQa += (uint32_t)__popcll(qa & lm);
        tQu += (uint32_t)__popcll(~qr & ~qa & lm);
        tUn += sumU;
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
                uint32_t A = 0, U = 0;
                for (uint32_t rr = 0; rr < L; ++rr) {
                    const uint32_t* d = reinterpret_cast<const uint32_t*>(dec + rr * 64u + q);
                    A |= ((d[half] >> sh) & 1u) << rr;
                    U |= ((d[2u + half] >> sh) & 1u) << rr;
                }
                const TrialResult res = trial_result(n, (uint32_t)ME, g.fmask, oc, A << 1, U << 1);
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
    const uint64_t Un = enum_wave_sum(tUn), Vi = enum_wave_sum(tVi), At = enum_wave_sum(tAt);
    uint64_t tot[C_NUM];
    tot[C_TRIALS] = T;
    tot[C_AGREE] = Ag;
    tot[C_VAPPL] = F0 ? 0ull : T;  // F, and with it in-bound and the faulty count, is the call's
    tot[C_VALID] = Va;
    tot[C_QR] = Qr;
    tot[C_QA] = Qa;
    tot[C_QU] = Qu;
    tot[C_UNDEF] = Un;
    tot[C_INB] = inb ? T : 0ull;
    tot[C_VIOL] = inb ? Vi : 0ull;
    tot[C_FTOT] = (uint64_t)nf * T;
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

template <int ME>
static hipError_t launch_enum_me(const RunArgs& a, const EnumCase& g, const uint8_t* d_map,
                                 uint64_t* witness, uint32_t blocks, uint32_t threads, uint32_t lds) {
    hipLaunchKernelGGL((k_enum<ME>), dim3(blocks), dim3(threads), lds, a.stream, g, a.first_trial,
                       a.batch, d_map, a.decisions, a.outcome, a.counters,
                       (unsigned long long*)witness, a.sink);
    return hipGetLastError();
}

// One persistent launch: a wave per tile of 64 words (4,096 strategies), at most
// kEnumBlocksPerCu four-wave blocks per CU; one counter-sink unit per wave.  With
// per-trial outputs the blocks are one wave each and hold L x 64 decision-plane
// pairs in LDS after the map (<= 4 KiB + 31 KiB).
hipError_t launch_enum(const RunArgs& a, const EnumCase& g, const uint8_t* d_map, uint64_t* witness) {
    if (a.n < 1 || a.n > (uint32_t)kMaxN || a.me > 8 || a.batch == 0 || g.map_bytes > kEnumMaxSlots ||
        (g.map_bytes & 15u))
        return hipErrorInvalidValue;
    const bool want_out = a.decisions != nullptr || a.outcome != nullptr;
    const uint32_t threads = want_out ? 64u : (uint32_t)kEnumThreads, wpb = threads / 64u;
    const uint32_t lds = g.map_bytes + (want_out ? (a.n - 1u) * 64u * (uint32_t)sizeof(EnumPair) : 0u);
    const uint64_t words = (a.batch + 63) / 64, tiles = (words + 63) / 64;
    uint64_t blocks = (tiles + wpb - 1) / wpb;
    const uint64_t cap = (uint64_t)kEnumBlocksPerCu * a.cu_count * (kEnumThreads / threads);
    if (blocks > cap) blocks = cap;
    ProfScope ps(a.prof, "k_enum", a.stream);
    switch (a.me) {
        case 0: return launch_enum_me<0>(a, g, d_map, witness, (uint32_t)blocks, threads, lds);
        case 1: return launch_enum_me<1>(a, g, d_map, witness, (uint32_t)blocks, threads, lds);
        case 2: return launch_enum_me<2>(a, g, d_map, witness, (uint32_t)blocks, threads, lds);
        case 3: return launch_enum_me<3>(a, g, d_map, witness, (uint32_t)blocks, threads, lds);
        case 4: return launch_enum_me<4>(a, g, d_map, witness, (uint32_t)blocks, threads, lds);
        case 5: return launch_enum_me<5>(a, g, d_map, witness, (uint32_t)blocks, threads, lds);
        case 6: return launch_enum_me<6>(a, g, d_map, witness, (uint32_t)blocks, threads, lds);
        case 7: return launch_enum_me<7>(a, g, d_map, witness, (uint32_t)blocks, threads, lds);
        default: return launch_enum_me<8>(a, g, d_map, witness, (uint32_t)blocks, threads, lds);
    }
}

}  // namespace ba
