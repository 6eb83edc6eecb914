// ba_adv.hip -- OM(m) under scripted traitor policies (docs/SEMANTICS.md §7):
// k_adv (gfx950).  A faulty sender does not flip a coin, it shows each recipient
// a face chosen by the policy, so the kernel draws no lie at all and the relay
// tree is never materialised.
//
// Bit-sliced: one 64-bit plane = one value for the 64 trials of a word.  A work
// item is (word, receiver r), one per thread; a block takes wpb consecutive words
// (wpb L <= 256 items, L = n-1).  Lieutenant r's root decision is a depth-first
// walk of its relay chains sigma (r not in sigma).  The walk carries
//   x   the truth plane L_{k-1}[sigma], what sigma's last lieutenant holds
//   Fs  the faulty plane of that lieutenant (the sender of every message below)
// and a node costs
//   the step to a child j    x' = L_k[sigma j]   = Fs ? face_k(j, x) : x
//   the node's own value     val = L_k[sigma r]  = Fs ? face_k(r, x) : x
//   one carry-save add of the child's result into the node's 5-plane counter
//   (leaves, most of the tree, go in pairs through a two-level carry-save adder).
// The faces are per-recipient planes staged once per word in LDS, in 16-byte
// pairs {F[j+1], G_k[j]} so a step is one ds_read_b128:
//   SPLIT  G_k[j] = j odd ? ~0 : 0                 at every level
//   ANTI   G_0[j] as SPLIT,  G_k[j] = ~L_0[j]      for k >= 1
//   FLIP   face = ~x, i.e. x' = x ^ Fs: no table, only F[j+1] is read
// Children are taken in the rank order of the lieutenants still free (lowest
// set bit of a mask), so every lane of a wave runs the same trip counts
// whatever its r.  The depth me is a template parameter (the recursion is
// inlined: the stack of counters lives in VGPRs), n is a runtime value.
//
// Per block and pass: stage (lane = trial: inputs loaded or drawn, planes by
// ballot) -> walk (lane = item) -> epilogue (lane = trial: decision planes
// picked out of LDS, trial_result, counters).  HBM traffic is the 5 B in and
// 9 B out per trial.
#include "ba_wave_proto.hpp"

namespace ba {

constexpr int kAdvThreads = 256;
constexpr uint32_t kAdvMaxWpb = 32;  // words per block (8 per wave in stage / epilogue)
constexpr uint32_t kAdvBlocksPerCu = 8;

struct __attribute__((aligned(16))) AdvPair {
    uint64_t a, b;
};

// LDS bytes of a block of wpb words: three pair tables of L entries per word
// ({F, G_0}, {F, G_>=1}, {attack, undefined} decision planes), the commander's
// {F[0], order} planes, and the trials' masks and order codes for the epilogue
__host__ __device__ inline uint32_t adv_lds_bytes(uint32_t wpb, uint32_t L) {
    return wpb * (3u * L * 16u + 16u + 64u * 4u + 64u);
}
__host__ inline uint32_t adv_wpb(uint32_t L) {
    if (L == 0) return kAdvThreads / 64;
    const uint32_t w = (uint32_t)kAdvThreads / L;
    return w < kAdvMaxWpb ? w : kAdvMaxWpb;
}

__device__ __forceinline__ uint64_t adv_sel(uint64_t f, uint64_t g, uint64_t x) {
    return (f & g) | (~f & x);
}

// resolve_r(sigma) of §2.3 for |sigma| = K under §7's face rule.  tab0 / tab1: the
// word's {F[j+1], G_0[j]} / {F[j+1], G_>=1[j]} tables; g0r, g1r: the receiver's own
// faces; free: lieutenants neither in sigma nor r.  tie (K == 0 only): the root's
// undefined plane.
template <int K, int ME, bool FLIP>
__device__ __forceinline__ uint64_t adv_resolve(const AdvPair* __restrict__ tab0,
                                                const AdvPair* __restrict__ tab1, uint64_t x,
                                                uint64_t Fs, uint64_t g0r, uint64_t g1r,
                                                uint32_t free, uint32_t L, uint64_t& tie) {
    const uint64_t val = FLIP ? x ^ Fs : adv_sel(Fs, K == 0 ? g0r : g1r, x);
    if constexpr (K == ME) {
        return val;
    } else {
        const AdvPair* __restrict__ tab = K == 0 ? tab0 : tab1;
        const uint32_t nch = L - 1u - (uint32_t)K;  // uniform: popcount(free)
        Count<5> cnt;  // L - K <= 31 inputs
        cnt.c[0] = val;
        uint32_t it = free;
        if constexpr (K + 1 == ME) {
            // The children are leaves, most of the tree: two at a time through one
            // full adder with plane 0 (carry-save), every second carry through one
            // with plane 1, and only that one's carry ripples into planes 2-4.
            auto leaf = [&]() {
                const uint32_t j = (uint32_t)__builtin_ctz(it);
                it &= it - 1u;
                if constexpr (FLIP) {
                    return x ^ Fs ^ tab[j].a;
                } else {
                    const AdvPair p = tab[j];
                    return adv_sel(p.a, g1r, adv_sel(Fs, p.b, x));  // the leaf's level is ME >= 1
                }
            };
            const uint32_t npairs = nch >> 1;
            uint64_t pend1 = 0;
            for (uint32_t q = 0; q < npairs; ++q) {
                const uint64_t e0 = leaf(), e1 = leaf();
                const uint64_t c1 = maj3(cnt.c[0], e0, e1);
                cnt.c[0] = xor3(cnt.c[0], e0, e1);
                if (q & 1u) {
                    uint64_t carry = maj3(cnt.c[1], pend1, c1);
                    cnt.c[1] = xor3(cnt.c[1], pend1, c1);
#pragma unroll
                    for (int i = 2; i < 5; ++i) {
                        const uint64_t t = cnt.c[i] & carry;
                        cnt.c[i] ^= carry;
                        carry = t;
                    }
                } else {
                    pend1 = c1;
                }
            }
            if (npairs & 1u) {  // a carry still pending: into planes 1-4
                uint64_t carry = pend1;
#pragma unroll
                for (int i = 1; i < 5; ++i) {
                    const uint64_t t = cnt.c[i] & carry;
                    cnt.c[i] ^= carry;
                    carry = t;
                }
            }
            if (nch & 1u) cnt.add(leaf());
        } else {
            uint64_t pend = 0;
            for (uint32_t c = 0; c < nch; ++c) {
                const uint32_t j = (uint32_t)__builtin_ctz(it);
                it &= it - 1u;
                uint64_t Fj, xc;
                if constexpr (FLIP) {
                    Fj = tab[j].a;
                    xc = x ^ Fs;
                } else {
                    const AdvPair p = tab[j];
                    Fj = p.a;
                    xc = adv_sel(Fs, p.b, x);
                }
                uint64_t dummy;
                const uint64_t e = adv_resolve<K + 1, ME, FLIP>(tab0, tab1, xc, Fj, g0r, g1r,
                                                                free ^ (1u << j), L, dummy);
                if (c & 1u) {  // carry-save: two results and plane 0 through one full adder
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
        }
        const uint32_t s = L - (uint32_t)K;  // inputs; strict majority = more than s / 2
        const uint64_t maj = cnt.ge(s / 2u + 1u);
        if constexpr (K == 0) tie = (s & 1u) ? 0ull : (cnt.ge(s / 2u) & ~maj);
        return maj;
    }
}

template <int ME, bool FLIP>
__global__ __launch_bounds__(kAdvThreads) void k_adv(uint32_t n, uint32_t anti, uint32_t wpb,
                                                     uint64_t seed, GenSpec gen,
                                                     uint64_t first_trial, uint64_t batch,
                                                     const uint32_t* __restrict__ faulty,
                                                     const uint8_t* __restrict__ order,
                                                     uint64_t* __restrict__ decisions,
                                                     uint8_t* __restrict__ outcome,
                                                     uint64_t* __restrict__ counters, Sink sk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char adv_lds[];
    const uint32_t L = n - 1;  // n = 1: no lieutenant, no item
    AdvPair* const tab0 = reinterpret_cast<AdvPair*>(adv_lds);  // [wpb][L] {F[j+1], G_0[j]}
    AdvPair* const tab1 = tab0 + wpb * L;                       // [wpb][L] {F[j+1], G_>=1[j]}
    AdvPair* const dec = tab1 + wpb * L;                        // [wpb][L] {attack, undefined}
    AdvPair* const hdr = dec + wpb * L;                         // [wpb]    {F[0], order == attack}
    uint32_t* const fms = reinterpret_cast<uint32_t*>(hdr + wpb);  // [wpb][64]
    uint8_t* const ocs = reinterpret_cast<uint8_t*>(fms + wpb * 64u);  // [wpb][64]
    const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const uint32_t all = general_mask(n);
    const uint64_t words = (batch + 63) / 64, nblk = (words + wpb - 1) / wpb;
    const uint32_t nwaves = gridDim.x * (kAdvThreads / 64), gwave = blockIdx.x * (kAdvThreads / 64) + wv;
    // this thread's item: receiver r of the block's word lw
    const uint32_t lw = L ? tid / L : 0u, r = L ? tid - lw * L : 0u;
    const bool item = L != 0 && lw < wpb;
    uint64_t mine = 0;
    for (uint64_t wb = blockIdx.x; wb < nblk; wb += gridDim.x) {
        const uint64_t w0 = wb * wpb;
        // stage, lane = trial: the word's planes and the trials' inputs
        for (uint32_t q = wv; q < wpb; q += kAdvThreads / 64) {
            const uint64_t i = (w0 + q) * 64 + lane;
            const bool live = w0 + q < words && i < batch;
            uint32_t fm, oc;
            trial_inputs<true>(live, n, all, seed, gen, first_trial, i, faulty, order, fm, oc);
            const uint64_t F0 = __ballot((fm & 1u) != 0), OB = __ballot(oc == 1);
            uint64_t myF = 0;
            for (uint32_t g = 1; g < n; ++g) {
                const uint64_t pl = faulty_plane(fm, g);
                if (lane == g - 1) myF = pl;
            }
            if (lane < L) {
                const uint64_t G0 = (lane & 1u) ? ~0ull : 0ull;
                const uint64_t G1 = anti ? ~adv_sel(F0, G0, OB) : G0;  // ANTI: the opposite of L_0[j]
                tab0[q * L + lane] = AdvPair{myF, G0};
                tab1[q * L + lane] = AdvPair{myF, G1};
            }
            if (lane == 0) hdr[q] = AdvPair{F0, OB};
            fms[q * 64u + lane] = fm;
            ocs[q * 64u + lane] = (uint8_t)oc;
        }
        __syncthreads();
        // walk, lane = item
        if (item) {
            const AdvPair h = hdr[lw];
            const AdvPair* const t0 = tab0 + lw * L;
            const AdvPair* const t1 = tab1 + lw * L;
            const uint64_t g0r = FLIP ? 0ull : t0[r].b, g1r = FLIP ? 0ull : t1[r].b;
            const uint32_t lts = general_mask(L);
            uint64_t tie = 0;
            const uint64_t A = adv_resolve<0, ME, FLIP>(t0, t1, h.b, h.a, g0r, g1r,
                                                        lts & ~(1u << r), L, tie);
            dec[lw * L + r] = AdvPair{A, tie};
        }
        __syncthreads();
        // epilogue, lane = trial: root decisions, quorum, flags
        for (uint32_t q = wv; q < wpb; q += kAdvThreads / 64) {
            const uint64_t i = (w0 + q) * 64 + lane;
            const bool live = w0 + q < words && i < batch;
            const uint32_t fm = fms[q * 64u + lane], oc = ocs[q * 64u + lane];
            uint32_t A = 0, U = 0;
            {
                const uint32_t half = lane >> 5, sh = lane & 31;
                const uint32_t* d = reinterpret_cast<const uint32_t*>(dec + q * L);
                for (uint32_t rr = 0; rr < L; ++rr) {
                    A |= ((d[rr * 4u + half] >> sh) & 1u) << rr;
                    U |= ((d[rr * 4u + 2u + half] >> sh) & 1u) << rr;
                }
            }
            const TrialResult res = trial_result(n, (uint32_t)ME, fm, oc, A << 1, U << 1);
            if (live) {
                if (decisions) decisions[i] = res.dec;
                if (outcome) outcome[i] = (uint8_t)res.out;
            }
            lane_counts_add<true>(live, res, lane, mine);
        }
        __syncthreads();  // the next pass restages the tables
    }
    sink_counters(lane, mine, gwave, nwaves, counters, sk);
}

template <int ME>
static hipError_t launch_adv_me(const RunArgs& a, uint32_t policy, uint32_t blocks, uint32_t wpb,
                                uint32_t lds) {
    const uint32_t anti = policy == 2 ? 1u : 0u;
    if (policy == 1)
        hipLaunchKernelGGL((k_adv<ME, true>), dim3(blocks), dim3(kAdvThreads), lds, a.stream, a.n, anti,
                           wpb, a.seed, a.gen, a.first_trial, a.batch, a.faulty, a.order, a.decisions,
                           a.outcome, a.counters, a.sink);
    else
        hipLaunchKernelGGL((k_adv<ME, false>), dim3(blocks), dim3(kAdvThreads), lds, a.stream, a.n, anti,
                           wpb, a.seed, a.gen, a.first_trial, a.batch, a.faulty, a.order, a.decisions,
                           a.outcome, a.counters, a.sink);
    return hipGetLastError();
}

// One launch for any batch: a persistent loop over blocks of wpb words, at most
// kAdvBlocksPerCu blocks per CU; one counter-sink unit per wave.
hipError_t launch_adv(const RunArgs& a, uint32_t policy) {
    if (a.n < 1 || a.n > (uint32_t)kMaxN || a.me > 8 || policy > 2 || a.batch == 0)
        return hipErrorInvalidValue;
    const uint32_t L = a.n - 1, wpb = adv_wpb(L), lds = adv_lds_bytes(wpb, L);
    const uint64_t words = (a.batch + 63) / 64;
    uint64_t blocks = (words + wpb - 1) / wpb;
    const uint64_t cap = (uint64_t)kAdvBlocksPerCu * a.cu_count;
    if (blocks > cap) blocks = cap;
    ProfScope ps(a.prof, "k_adv", a.stream);
    switch (a.me) {
        case 0: return launch_adv_me<0>(a, policy, (uint32_t)blocks, wpb, lds);
        case 1: return launch_adv_me<1>(a, policy, (uint32_t)blocks, wpb, lds);
        case 2: return launch_adv_me<2>(a, policy, (uint32_t)blocks, wpb, lds);
        case 3: return launch_adv_me<3>(a, policy, (uint32_t)blocks, wpb, lds);
        case 4: return launch_adv_me<4>(a, policy, (uint32_t)blocks, wpb, lds);
        case 5: return launch_adv_me<5>(a, policy, (uint32_t)blocks, wpb, lds);
        case 6: return launch_adv_me<6>(a, policy, (uint32_t)blocks, wpb, lds);
        case 7: return launch_adv_me<7>(a, policy, (uint32_t)blocks, wpb, lds);
        default: return launch_adv_me<8>(a, policy, (uint32_t)blocks, wpb, lds);
    }
}

}  // namespace ba
