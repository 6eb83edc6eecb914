// ba_sm.hip -- SM(m), Lamport's signed-messages algorithm in its Dolev-Strong
// form (docs/SEMANTICS.md §6), one 64-trial word per wave (k_sm, gfx950).
//
// A lieutenant keeps a set V of at most two values and, per value, a flag
// "fresh" (accepted in the previous round); messages carry no per-path state.
// Bit-sliced over the word that is four planes per lieutenant: hasR, hasA,
// freshR, freshA (bit b = trial 64 w + b).  Layout of a wave:
//   lane r < L          lieutenant r: its four planes in registers
//   lane b              trial b of the word for the inputs and the epilogue
//   lane l, pass q      (sender j, recipient r) pair p = 64 q + l in a relay round
// Per wave, in LDS (1,792 B; four waves per block, no block barrier):
//   F[j]                faulty plane of lieutenant j (ballots over the trials' masks)
//   fresh[v][j]         what the senders relay this round
//   recv[v][r]          what the recipients receive: the pair lanes OR
//                       fresh_v[j] & (~F[j] | coin_v) into it (64-bit LDS atomic OR)
//   has[v][r]           final V planes for the lane = trial epilogue
// The DS instructions of one wave execute in issue order, so between the
// phases only the compiler has to be held (wave_sync, ba_wave_proto.hpp).
//
// One Philox call (ctr word 1 = 64 + k) yields the retreat and attack coins of
// one pair for the 64 trials; a lane with several pairs groups up to four calls
// (philox10_n).  Two wave-uniform shortcuts, both invisible in the results:
// a round in which no lieutenant holds a fresh value ends the relay, and a
// group of pairs none of whose senders is both faulty and fresh in some trial
// draws no coins (a loyal sender's coin is never read).
#include "ba_wave_proto.hpp"

namespace ba {

constexpr uint32_t kSmTag = 64;  // Philox ctr word 1 of round k: kSmTag + k
constexpr int kSmThreads = 256;  // four independent waves
constexpr int kSmBlocksPerCu = 4;  // k_sm's 128 VGPRs: four waves per SIMD

struct SmWave {
    uint64_t F[kMaxN];
    uint64_t fresh[2][kMaxN];
    uint64_t recv[2][kMaxN];
    uint64_t has[2][kMaxN];
};

// One group of G relay passes of round k: lane l takes pairs base + 64 g + l.
template <int G>
__device__ __forceinline__ void sm_relay_group(SmWave& s, uint32_t lane, uint32_t base, uint32_t P,
                                               uint32_t L, const FastDiv& dL1, uint32_t k,
                                               uint64_t gw, uint64_t seed) {
    uint32_t p[G], r[G];
    uint64_t fR[G], fA[G], Fj[G];
    bool need = false;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        p[g] = base + (uint32_t)g * 64u + lane;
        const bool act = p[g] < P;
        const uint32_t pp = act ? p[g] : 0u;
        const uint32_t j = fdiv(pp, dL1), rr = pp - j * (L - 1);
        r[g] = rr + (rr >= j ? 1u : 0u);
        fR[g] = act ? s.fresh[0][j] : 0ull;
        fA[g] = act ? s.fresh[1][j] : 0ull;
        Fj[g] = s.F[j];
        need |= ((fR[g] | fA[g]) & Fj[g]) != 0;
    }
    uint64_t cR[G], cA[G];
#pragma unroll
    for (int g = 0; g < G; ++g) cR[g] = cA[g] = 0;
    if (__ballot(need) != 0) {
        const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
        if constexpr (G == 1) {
            const P4 o = philox10(P4{p[0], kSmTag + k, (uint32_t)gw, (uint32_t)(gw >> 32)}, k0, k1);
            cR[0] = (uint64_t)o.y << 32 | o.x;
            cA[0] = (uint64_t)o.w << 32 | o.z;
        } else {
            P4 c[G];
#pragma unroll
            for (int g = 0; g < G; ++g) c[g] = P4{p[g], kSmTag + k, (uint32_t)gw, (uint32_t)(gw >> 32)};
            philox10_n<G>(c, k0, k1);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                cR[g] = (uint64_t)c[g].y << 32 | c[g].x;
                cA[g] = (uint64_t)c[g].w << 32 | c[g].z;
            }
        }
    }
#pragma unroll
    for (int g = 0; g < G; ++g) {
        // an inactive lane's fresh words are zero: it sends nothing
        const uint64_t aR = fR[g] & (~Fj[g] | cR[g]), aA = fA[g] & (~Fj[g] | cA[g]);
        if (aR) lds_or(&s.recv[0][r[g]], aR);
        if (aA) lds_or(&s.recv[1][r[g]], aA);
    }
}

template <bool GEN>
__global__ __launch_bounds__(kSmThreads) void k_sm(uint32_t n, uint32_t m, uint32_t me, uint64_t seed,
                                                   GenSpec gen, FastDiv dL1, uint64_t first_trial,
                                                   uint64_t batch,
                                                   const uint32_t* __restrict__ faulty,
                                                   const uint8_t* __restrict__ order,
                                                   uint64_t* __restrict__ decisions,
                                                   uint8_t* __restrict__ outcome,
                                                   uint64_t* __restrict__ vsets,
                                                   uint64_t* __restrict__ counters, Sink sk) {
    __shared__ SmWave lds[kSmThreads / 64];
    const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    SmWave& s = lds[wv];
    const uint32_t L = n - 1, P = L * (L - 1);  // n = 1: L = 0, P = 0
    const uint32_t all = general_mask(n);
    const uint64_t words = (batch + 63) / 64;
    const uint32_t nwaves = gridDim.x * (kSmThreads / 64), gwave = blockIdx.x * (kSmThreads / 64) + wv;
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    uint64_t mine = 0;
    for (uint64_t w = gwave; w < words; w += nwaves) {
        const uint64_t i = w * 64 + lane, gw = (first_trial >> 6) + w;
        const bool live = i < batch;
        uint32_t fm, oc;
        trial_inputs<GEN>(live, n, all, seed, gen, first_trial, i, faulty, order, fm, oc);
        // planes of the word
        const uint64_t VAL = __ballot(live), F0 = __ballot((fm & 1u) != 0), OB = __ballot(oc == 1);
        for (uint32_t g = 1; g < n; ++g) {
            const uint64_t pl = faulty_plane(fm, g);
            if (lane == g - 1) s.F[g - 1] = pl;
        }
        // round 0: the commander sends; a faulty one signs each value by a coin
        uint64_t hasR = 0, hasA = 0, freshR = 0, freshA = 0;
        {
            uint64_t cR = 0, cA = 0;
            if (F0 != 0) {
                const P4 o = philox10(P4{lane, kSmTag, (uint32_t)gw, (uint32_t)(gw >> 32)}, k0, k1);
                cR = (uint64_t)o.y << 32 | o.x;
                cA = (uint64_t)o.w << 32 | o.z;
            }
            if (lane < L) {
                freshR = hasR = VAL & ((F0 & cR) | (~F0 & ~OB));
                freshA = hasA = VAL & ((F0 & cA) | (~F0 & OB));
            }
        }
        // rounds 1..me: every lieutenant relays its fresh values
        for (uint32_t k = 1; k <= me; ++k) {
            if (__ballot((freshR | freshA) != 0) == 0) break;  // nothing left to relay
            wave_sync();
            if (lane < L) {
                s.fresh[0][lane] = freshR;
                s.fresh[1][lane] = freshA;
                s.recv[0][lane] = 0;
                s.recv[1][lane] = 0;
            }
            wave_sync();
            uint32_t base = 0;
            for (; base + 192 < P; base += 256) sm_relay_group<4>(s, lane, base, P, L, dL1, k, gw, seed);
            if (base + 128 < P) sm_relay_group<3>(s, lane, base, P, L, dL1, k, gw, seed);
            else if (base + 64 < P) sm_relay_group<2>(s, lane, base, P, L, dL1, k, gw, seed);
            else if (base < P) sm_relay_group<1>(s, lane, base, P, L, dL1, k, gw, seed);
            wave_sync();
            if (lane < L) {
                freshR = s.recv[0][lane] & ~hasR;
                freshA = s.recv[1][lane] & ~hasA;
                hasR |= freshR;
                hasA |= freshA;
            }
        }
        // epilogue, lane = trial: V sets, choice(V), quorum, flags
        wave_sync();
        if (lane < L) {
            s.has[0][lane] = hasR;
            s.has[1][lane] = hasA;
        }
        wave_sync();
        uint32_t vR = 0, vA = 0;
        for (uint32_t r = 0; r < L; ++r) {
            vR |= lane_bit(&s.has[0][r], lane) << r;
            vA |= lane_bit(&s.has[1][r], lane) << r;
        }
        // §2.4's epilogue with the SM rules of §6: decisions are never undefined
        // (attack where V = {attack}) and in-bound is |F| <= m, no condition on n
        TrialResult res = trial_result(n, 0, fm, oc, (vA & ~vR) << 1, 0);
        res.out = (res.out & ~32u) | (res.nf <= m ? 32u : 0u);
        if (live) {
            if (decisions) decisions[i] = res.dec;
            if (outcome) outcome[i] = (uint8_t)res.out;
            if (vsets) vsets[i] = part1by1(vA) | part1by1(vR) << 1;
        }
        lane_counts_add<false>(live, res, lane, mine);
    }
    sink_counters(lane, mine, gwave, nwaves, counters, sk);
}

// One launch for any batch: a persistent word loop over at most kSmBlocksPerCu
// blocks per CU, one counter-sink unit per wave (4,096 on 256 CUs: 64 per
// replica, far below the sink's 2^16).
hipError_t launch_sm(const RunArgs& a, uint64_t* vsets) {
    if (a.n < 1 || a.n > (uint32_t)kMaxN || a.batch == 0) return hipErrorInvalidValue;
    constexpr uint32_t wpb = kSmThreads / 64;
    const uint64_t words = (a.batch + 63) / 64;
    uint64_t blocks = (words + wpb - 1) / wpb;
    const uint64_t cap = (uint64_t)kSmBlocksPerCu * a.cu_count;  // persistent word loop beyond
    if (blocks > cap) blocks = cap;
    const FastDiv dL1 = make_fastdiv(a.n >= 2 ? a.n - 2 : 0);
    const bool gen = a.gen.faulty_mode != 0 || a.gen.order_mode != 0;
    ProfScope ps(a.prof, "k_sm", a.stream);
    if (gen)
        hipLaunchKernelGGL(k_sm<true>, dim3((uint32_t)blocks), dim3(kSmThreads), 0, a.stream, a.n, a.m,
                           a.me, a.seed, a.gen, dL1, a.first_trial, a.batch, a.faulty, a.order,
                           a.decisions, a.outcome, vsets, a.counters, a.sink);
    else
        hipLaunchKernelGGL(k_sm<false>, dim3((uint32_t)blocks), dim3(kSmThreads), 0, a.stream, a.n,
                           a.m, a.me, a.seed, a.gen, dL1, a.first_trial, a.batch, a.faulty, a.order,
                           a.decisions, a.outcome, vsets, a.counters, a.sink);
    return hipGetLastError();
}

}  // namespace ba
