// ba_king_common.hpp -- device helpers shared by the two King kernels, k_king
// (ba_king.hip, docs/SEMANTICS.md §9) and k_king3 (ba_king3.hip, §10): both hold one
// 64-trial word per wave, lane (i, s) = recipient i and sender slice s, with
// wave-private LDS ordered by king_wave_sync.
#pragma once
#include "ba_engine.hpp"

namespace ba {

// orders this wave's LDS accesses for the compiler (no instruction: one wave's
// DS operations complete in order)
__device__ __forceinline__ void king_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void king_lds_or(uint64_t* p, uint64_t v) {
    (void)__hip_atomic_fetch_or((unsigned long long*)p, (unsigned long long)v, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the value of lane ^ 1 (DPP quad_perm [1,0,3,2])
__device__ __forceinline__ uint64_t swap_neighbour(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)v, 0xB1, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(v >> 32), 0xB1, 0xF, 0xF, false);
    return (uint64_t)hi << 32 | lo;
}

// Wave totals of one word's run counters added into `mine` (lane c holds
// counter c): flags by ballot + popcount, the small integers bit-sliced
// (faulty_total up to 32 per trial: six planes).
__device__ __forceinline__ void king_counts_add(bool live, const TrialResult& r, uint32_t lane,
                                                uint64_t& mine) {
    const uint32_t o = r.out, q = o & 3;
    const bool agree = (o >> 2) & 1, appl = (o >> 3) & 1, valid = (o >> 4) & 1, inb = (o >> 5) & 1;
    uint32_t c[C_NUM];
    c[C_TRIALS] = __popcll(__ballot(live));
    c[C_AGREE] = __popcll(__ballot(live && agree));
    c[C_VAPPL] = __popcll(__ballot(live && appl));
    c[C_VALID] = __popcll(__ballot(live && valid));
    c[C_QR] = __popcll(__ballot(live && q == 0));
    c[C_QA] = __popcll(__ballot(live && q == 1));
    c[C_QU] = __popcll(__ballot(live && q == 2));
    c[C_INB] = __popcll(__ballot(live && inb));
    c[C_VIOL] = __popcll(__ballot(live && inb && (!agree || (appl && !valid))));
    c[C_UNDEF] = c[C_FTOT] = c[C_ATT] = 0;
#pragma unroll
    for (int b = 0; b < 6; ++b) {
        c[C_FTOT] += (uint32_t)__popcll(__ballot(live && ((r.nf >> b) & 1u))) << b;
        c[C_ATT] += (uint32_t)__popcll(__ballot(live && ((r.nA >> b) & 1u))) << b;
    }
#pragma unroll
    for (int i = 0; i < C_NUM; ++i)
        if (lane == (uint32_t)i) mine += c[i];
}

// The coin words sender j shows this lane's recipient i, for the lane's own call
// (pair = 16 j + i / 2): `keep` is i's half, `give` that of recipient i ^ 1.
struct KingCoin {
    uint64_t keep, give;
};
__device__ __forceinline__ KingCoin king_halves(const P4& o, uint32_t odd) {
    const uint64_t even_r = (uint64_t)o.y << 32 | o.x, odd_r = (uint64_t)o.w << 32 | o.z;
    return KingCoin{odd ? odd_r : even_r, odd ? even_r : odd_r};
}

// The coin word a faulty sender j shows recipient i in round q of the protocol
// whose Philox tag is TAG (every lane draws its own copy of the pair's call: one
// call deep, whatever n).
template <bool COIN, uint32_t TAG>
__device__ __forceinline__ uint64_t king_one_coin(uint32_t j, uint32_t i, uint32_t q, uint64_t gw,
                                                  uint64_t seed) {
    if constexpr (COIN) {
        const P4 o = philox10(P4{16u * j + (i >> 1), TAG + q, (uint32_t)gw, (uint32_t)(gw >> 32)},
                              (uint32_t)seed, (uint32_t)(seed >> 32));
        return king_halves(o, i & 1u).keep;
    } else {
        return (i & 1u) ? ~0ull : 0ull;
    }
}

// Bit `lane` of: do the loyal generals hold one common preference?  (lanes i < n
// of slice 0 contribute; `pref` and `myF` are general i's planes; Wave has the
// two LDS words agr[2])
template <class Wave>
__device__ __forceinline__ bool king_agree(Wave& s, uint32_t lane, uint32_t n, uint64_t pref,
                                           uint64_t myF) {
    king_wave_sync();
    if (lane == 0) s.agr[0] = s.agr[1] = 0;
    king_wave_sync();
    if (lane < n) {
        king_lds_or(&s.agr[1], pref & ~myF);
        king_lds_or(&s.agr[0], ~pref & ~myF);
    }
    king_wave_sync();
    const uint64_t split = s.agr[0] & s.agr[1];
    return ((split >> lane) & 1ull) == 0;
}

}  // namespace ba
