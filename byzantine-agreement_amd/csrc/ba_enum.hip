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
// The tile loop, the counters (IC1 / IC2 by AND over the loyal receivers' {attack,
// undefined, retreat} planes), the witness and the per-trial outputs are the frame
// of ba_enum_common.hpp, here with the second, undefined plane; the word evaluator
// below hands it each receiver's pair of planes.
#include "ba_enum_common.hpp"

namespace ba {

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
    // the slot map: g.map_bytes (a multiple of 16) bytes of the ctx's scratch -> LDS;
    // the decision planes follow it
    for (uint32_t i = threadIdx.x * 4u; i < g.map_bytes; i += blockDim.x * 4u)
        *reinterpret_cast<uint32_t*>(enum_lds + i) = *reinterpret_cast<const uint32_t*>(map + i);
    __syncthreads();

    EnumWalk c;
    c.map = enum_lds;
#pragma unroll
    for (int k = 0; k < kEnumLevels; ++k) c.off[k] = g.off[k];
    c.L = L;
    c.fl = g.fmask >> 1;
    const bool F0 = (g.fmask & 1u) != 0;
    const uint64_t ob = g.order == 1u ? ~0ull : 0ull;
    const uint32_t lts = general_mask(L);
    const bool inb = (uint32_t)__popc(g.fmask) <= (uint32_t)ME && n > 3u * (uint32_t)ME;
    const EnumRun run{n, g.fmask, g.order, (uint32_t)ME, inb, first_trial, batch, decisions, outcome,
                      counters, witness};
    enum_frame<true, false>(run, enum_lds + g.map_bytes, sk,
                            [&](uint32_t wlo, uint32_t whi, EnumTally<true>& ty) {
        c.wlo = wlo;
        c.whi = whi;
        for (uint32_t r = 0; r < L; ++r) {
            c.r = r;
            uint64_t U = 0;
            const uint64_t A = enum_resolve<0, ME>(c, ob, F0, 0u, lts, U);
            ty.put(r, !((c.fl >> r) & 1u), A, U);
        }
    });
}

template <int ME>
static hipError_t launch_enum_me(const RunArgs& a, const EnumCase& g, const uint8_t* d_map,
                                 uint64_t* witness, uint32_t blocks, uint32_t threads, uint32_t lds) {
    hipLaunchKernelGGL((k_enum<ME>), dim3(blocks), dim3(threads), lds, a.stream, g, a.first_trial,
                       a.batch, d_map, a.decisions, a.outcome, a.counters,
                       (unsigned long long*)witness, a.sink);
    return hipGetLastError();
}

// One persistent launch of enum_geometry's shape: the decision-plane pairs follow the
// map in LDS (<= 4 KiB + 31 KiB).
hipError_t launch_enum(const RunArgs& a, const EnumCase& g, const uint8_t* d_map, uint64_t* witness) {
    if (a.n < 1 || a.n > (uint32_t)kMaxN || a.me > 8 || a.batch == 0 || g.map_bytes > kEnumMaxSlots ||
        (g.map_bytes & 15u))
        return hipErrorInvalidValue;
    const EnumGeometry ge = enum_geometry(a, (uint32_t)sizeof(EnumEntry<true>), g.map_bytes);
    const uint32_t blocks = ge.blocks, threads = ge.threads, lds = ge.lds;
    ProfScope ps(a.prof, "k_enum", a.stream);
    switch (a.me) {
        case 0: return launch_enum_me<0>(a, g, d_map, witness, blocks, threads, lds);
        case 1: return launch_enum_me<1>(a, g, d_map, witness, blocks, threads, lds);
        case 2: return launch_enum_me<2>(a, g, d_map, witness, blocks, threads, lds);
        case 3: return launch_enum_me<3>(a, g, d_map, witness, blocks, threads, lds);
        case 4: return launch_enum_me<4>(a, g, d_map, witness, blocks, threads, lds);
        case 5: return launch_enum_me<5>(a, g, d_map, witness, blocks, threads, lds);
        case 6: return launch_enum_me<6>(a, g, d_map, witness, blocks, threads, lds);
        case 7: return launch_enum_me<7>(a, g, d_map, witness, blocks, threads, lds);
        default: return launch_enum_me<8>(a, g, d_map, witness, blocks, threads, lds);
    }
}

}  // namespace ba
