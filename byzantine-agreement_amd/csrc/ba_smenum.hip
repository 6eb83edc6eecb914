// ba_smenum.hip -- SM(m) against EVERY strategy of a traitor coalition that shares
// its signatures (docs/SEMANTICS.md §12): k_smenum (gfx950).  One case is (form, n,
// m, faulty set F, order o); every message the coalition can validly deliver to a
// loyal lieutenant is a free bit (1 = sent), a strategy S is an assignment of the B
// free bits, and trial t of a call is strategy S = t.  The kernel draws nothing,
// loads no per-trial input and reads no table: there is nothing to upload.
//
// k_kenum's stance (ba_kenum.hip): one LANE holds one 64-strategy word w = S / 64,
// a wave takes a tile of 64 consecutive words.  F, l (loyal lieutenants), fL (faulty
// lieutenants), K = min(me, fL), c = [0 in F] and with them the index of every free
// bit,
//   round 0 (c = 1)   2 lr + v
//   round k = 1..K    c 2l + (k - 1) per + (jr l + lr)(1 + c) + c v    (messages)
//                     c 2l + (k - 1) per +        lr (1 + c) + c v    (coalition)
// (lr, jr: ranks among the loyal / the faulty lieutenants; per: a round's bits),
// are wave-uniform: SGPR arithmetic and scalar branches.
//
// State per lane: has[v][lr] for every loyal lieutenant, by loyal rank in register
// arrays of the padded length LP (a template parameter; full unroll, uniform guards
// lr < l, so nothing is indexed dynamically), and two planes anyfresh[v].  A loyal
// relay goes to everyone, so what recipient lr is shown in round k is
//   recv[v] = anyfresh[v] | (its free planes of round k, k <= K)
// and new = recv & ~has, anyfresh' = OR of new over the loyal lieutenants.  No fresh
// plane per lieutenant is needed: a lieutenant that is the only fresh one of a value
// holds it.  The faulty lieutenants keep one V between them, two planes: the loyal
// commander's value and whatever a loyal lieutenant relayed.
//
// All 12 counters come from planes, per lane = word; the witness is the wave's lowest
// violating S, one 64-bit atomic min per wave that found one.  The lane = trial
// pick-out of decisions / outcome bytes runs only when asked for, on one-wave blocks
// that keep the tile's decision planes in LDS.
#include "ba_enum_common.hpp"

namespace ba {

constexpr int kSmenumThreads = 256;
constexpr uint32_t kSmenumBlocksPerCu = 8;
constexpr uint32_t kSmenumPad = 8;  // LP is a multiple of it: 8, 16, 24, 32

template <int FORM, int LP>
__global__ __launch_bounds__(kSmenumThreads) void k_smenum(SmenumCase g, uint64_t first_trial,
                                                           uint64_t batch,
                                                           uint64_t* __restrict__ decisions,
                                                           uint8_t* __restrict__ outcome,
                                                           uint64_t* __restrict__ counters,
                                                           unsigned long long* __restrict__ witness,
                                                           Sink sk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smenum_lds[];
    const uint32_t n = g.n, L = n - 1u;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t wpb = blockDim.x >> 6;
    const uint32_t wv = (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6));
    const bool want_out = decisions != nullptr || outcome != nullptr;  // then wpb == 1 (launch_smenum)
    uint64_t* const dec = reinterpret_cast<uint64_t*>(smenum_lds);     // [L][64], want_out only

    const uint32_t F = g.fmask;
    const uint32_t lts = (n >= 32u ? 0xFFFFFFFFu : ((1u << n) - 1u)) & ~1u;
    const bool F0 = (F & 1u) != 0;
    const uint32_t nf = (uint32_t)__popc(F), fL = (uint32_t)__popc(F & lts), l = L - fL;
    const uint32_t K = g.me < fL ? g.me : fL;
    const uint32_t two = F0 ? 2u : 1u;                       // bits of one (sender, recipient)
    const uint32_t per = (FORM == 0 ? fL : 1u) * l * two;    // bits of one relay round
    const uint32_t rbase = F0 ? 2u * l : 0u;                 // first bit of round 1
    const uint32_t oc = g.order;
    const uint32_t obv = oc == 1u ? 1u : 0u;
    const uint64_t ob = obv ? ~0ull : 0ull;
    // quorum thresholds (§2.4): every general answers, total = n
    uint32_t needed = 2u * ((n - 1u) / 3u) + 1u;
    if (n <= 3u) needed = n - 1u;
    if (n == 1u) needed = 1u;
    const uint32_t needA = needed - (oc == 1u ? 1u : 0u);                        // attack iff nA >= needA
    const int32_t maxN = (int32_t)(L + (oc == 0u ? 1u : 0u)) - (int32_t)needed;  // retreat iff nA <= maxN
    const bool inb = nf <= g.m;

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
        const uint32_t wlo = (uint32_t)gw, whi = (uint32_t)(gw >> 32);
        // round 0: the commander sends
        uint64_t has0[LP], has1[LP];
        uint64_t af0 = 0, af1 = 0;             // some loyal lieutenant accepted v in the last round
        uint64_t V0 = F0 ? 0ull : ~ob, V1 = F0 ? 0ull : ob;  // the faulty lieutenants' V
#pragma unroll
        for (int lr = 0; lr < LP; ++lr) {
            has0[lr] = has1[lr] = 0;
            if ((uint32_t)lr < l) {
                has0[lr] = F0 ? enum_plane(2u * (uint32_t)lr, wlo, whi) : ~ob;
                has1[lr] = F0 ? enum_plane(2u * (uint32_t)lr + 1u, wlo, whi) : ob;
                af0 |= has0[lr];
                af1 |= has1[lr];
            }
        }
        // rounds 1..me: loyal relays of what was fresh, and the coalition's free messages
        uint32_t base = rbase;
        for (uint32_t k = 1; k <= g.me; ++k) {
            V0 |= af0;  // a loyal relay reaches the traitors too
            V1 |= af1;
            const bool open = k <= K;
            uint64_t n0 = 0, n1 = 0;
#pragma unroll
            for (int lr = 0; lr < LP; ++lr) {
                if ((uint32_t)lr < l) {
                    uint64_t r0 = af0, r1 = af1;
                    if (open) {
                        if constexpr (FORM == 0) {
                            for (uint32_t jr = 0; jr < fL; ++jr) {
                                const uint32_t b = base + (jr * l + (uint32_t)lr) * two;
                                if (F0) {
                                    r0 |= enum_plane(b, wlo, whi);
                                    r1 |= enum_plane(b + 1u, wlo, whi);
                                } else if (obv) {
                                    r1 |= enum_plane(b, wlo, whi);
                                } else {
                                    r0 |= enum_plane(b, wlo, whi);
                                }
                            }
                        } else {
                            const uint32_t b = base + (uint32_t)lr * two;
                            if (F0) {
                                r0 |= enum_plane(b, wlo, whi);
                                r1 |= enum_plane(b + 1u, wlo, whi);
                            } else if (obv) {
                                r1 |= enum_plane(b, wlo, whi);
                            } else {
                                r0 |= enum_plane(b, wlo, whi);
                            }
                        }
                    }
                    const uint64_t new0 = r0 & ~has0[lr], new1 = r1 & ~has1[lr];
                    has0[lr] |= new0;
                    has1[lr] |= new1;
                    n0 |= new0;
                    n1 |= new1;
                }
            }
            af0 = n0;
            af1 = n1;
            if (open) base += per;
        }
        // decisions = choice(V): attack iff V = {attack}; never undefined
        const uint64_t Af = V1 & ~V0;  // every faulty lieutenant's
        uint64_t allA = ~0ull, allR = ~0ull;
        Count<5> cA;
        uint32_t sumA = fL * (uint32_t)__popcll(Af & lm);
        uint32_t rest = ~F & lts;  // the loyal lieutenants not yet met, in ascending index
#pragma unroll
        for (int lr = 0; lr < LP; ++lr) {
            if ((uint32_t)lr < l) {
                const uint64_t A = has1[lr] & ~has0[lr];
                allA &= A;
                allR &= ~A;
                cA.add(A);
                sumA += (uint32_t)__popcll(A & lm);
                if (want_out) dec[((uint32_t)__builtin_ctz(rest) - 1u) * 64u + lane] = A;
                rest &= rest - 1u;
            }
        }
        for (uint32_t fm = F & lts; fm; fm &= fm - 1u) {
            cA.add(Af);
            if (want_out) dec[((uint32_t)__builtin_ctz(fm) - 1u) * 64u + lane] = Af;
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
                TrialResult res = trial_result(n, 0, F, oc, A << 1, 0);
                res.out = (res.out & ~32u) | (inb ? 32u : 0u);  // in-bound is SM's: |F| <= m
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

using SmenumKernel = void (*)(SmenumCase, uint64_t, uint64_t, uint64_t*, uint8_t*, uint64_t*,
                              unsigned long long*, Sink);

template <int FORM>
static SmenumKernel smenum_kernel_of(uint32_t l) {
    static constexpr SmenumKernel tab[] = {k_smenum<FORM, 8>, k_smenum<FORM, 16>, k_smenum<FORM, 24>,
                                           k_smenum<FORM, 32>};
    return tab[l <= kSmenumPad ? 0u : (l - 1u) / kSmenumPad];
}

// One persistent launch: a wave per tile of 64 words (4,096 strategies), at most
// kSmenumBlocksPerCu four-wave blocks per CU; one counter-sink unit per wave.  With
// per-trial outputs the blocks are one wave each and hold (n - 1) x 64 decision
// planes in LDS (at most 15.5 KiB).  The kernel is picked by the loyal lieutenants'
// count, padded to a multiple of kSmenumPad.
hipError_t launch_smenum(const RunArgs& a, const SmenumCase& g, uint64_t* witness) {
    if (a.n < 1 || a.n > 32 || g.n != a.n || g.form > 1 || a.batch == 0 || g.me > a.n)
        return hipErrorInvalidValue;
    const uint32_t lts = (a.n >= 32u ? 0xFFFFFFFFu : ((1u << a.n) - 1u)) & ~1u;
    if (g.fmask & ~(lts | 1u)) return hipErrorInvalidValue;
    const uint32_t l = a.n - 1u - (uint32_t)__builtin_popcount(g.fmask & lts);
    const bool want_out = a.decisions != nullptr || a.outcome != nullptr;
    const uint32_t threads = want_out ? 64u : (uint32_t)kSmenumThreads, wpb = threads / 64u;
    const uint32_t lds = want_out ? (a.n - 1u) * 64u * (uint32_t)sizeof(uint64_t) : 0u;
    const uint64_t words = (a.batch + 63) / 64, tiles = (words + 63) / 64;
    uint64_t blocks = (tiles + wpb - 1) / wpb;
    const uint64_t cap = (uint64_t)kSmenumBlocksPerCu * a.cu_count * (kSmenumThreads / threads);
    if (blocks > cap) blocks = cap;
    ProfScope ps(a.prof, "k_smenum", a.stream);
    const SmenumKernel k = g.form == 0 ? smenum_kernel_of<0>(l) : smenum_kernel_of<1>(l);
    hipLaunchKernelGGL(k, dim3((uint32_t)blocks), dim3(threads), lds, a.stream, g, a.first_trial, a.batch,
                       a.decisions, a.outcome, a.counters, (unsigned long long*)witness, a.sink);
    return hipGetLastError();
}

}  // namespace ba
