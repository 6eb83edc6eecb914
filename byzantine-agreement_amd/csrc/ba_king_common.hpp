// ba_king_common.hpp -- device helpers of the two King kernels alone, k_king
// (ba_king.hip, docs/SEMANTICS.md §9) and k_king3 (ba_king3.hip, §10): both hold one
// 64-trial word per wave, lane (i, s) = recipient i and sender slice s.  What they
// share with the other word-per-wave kernels is ba_wave_proto.hpp's.
#pragma once
#include "ba_wave_proto.hpp"

namespace ba {

// the value of lane ^ 1 (DPP quad_perm [1,0,3,2])
__device__ __forceinline__ uint64_t swap_neighbour(uint64_t v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)v, 0xB1, 0xF, 0xF, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_mov_dpp((int)(uint32_t)(v >> 32), 0xB1, 0xF, 0xF, false);
    return (uint64_t)hi << 32 | lo;
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
    wave_sync();
    if (lane == 0) s.agr[0] = s.agr[1] = 0;
    wave_sync();
    if (lane < n) {
        lds_or(&s.agr[1], pref & ~myF);
        lds_or(&s.agr[0], ~pref & ~myF);
    }
    wave_sync();
    const uint64_t split = s.agr[0] & s.agr[1];
    return ((split >> lane) & 1ull) == 0;
}

}  // namespace ba
