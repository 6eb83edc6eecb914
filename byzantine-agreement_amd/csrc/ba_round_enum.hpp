// ba_round_enum.hpp -- what the round-based enumerations share: k_kenum (ba_kenum.hip,
// docs/SEMANTICS.md §11) and k_renum (ba_renum.hip, §14), on the frame of
// ba_enum_common.hpp.  One LANE holds one 64-strategy word w = S / 64 and the planes
// of its N generals in registers (N is a template parameter, so the plane arrays are
// never indexed dynamically).  F and the round are wave-uniform, and with them the
// class of every message (truth / free / dead) and the index of its free bit,
//   base of the round + rank of the sender among the traitors * l
//                     + rank of the recipient among the loyal      (l = n - |F|),
// doubled for a two-bit proposal (lo, hi): SGPR arithmetic and scalar branches.
//
// A round's tally at recipient i splits into what every recipient sees alike, the
// loyal senders' true values, counted once per round (round_loyal), and what only i
// sees:
//   i loyal    the |F| free planes addressed to it, by traitor rank
//   i faulty   its own true value; the other traitors' messages are dead
//              (retreat / no proposal) and add nothing
// So the sender's identity never matters, only its rank, and a recipient's update
// needs nobody else's plane of the same round: planes are updated in place.  The
// protocols' rules (thresholds, proposals, kings, coins) are their own files'.
#pragma once
#include "ba_enum_common.hpp"

#include <type_traits>

namespace ba {

using RoundCount = Count<5>;  // a tally of at most 16 messages

// The case (uniform over the launch) and the lane's word.
struct RoundWord {
    uint32_t F, nf, ell;  // the faulty mask, |F|, the loyal generals
    uint32_t wlo, whi;    // this lane's word index w = S / 64
};

__device__ __forceinline__ RoundWord round_word(uint32_t fmask, uint32_t n, uint32_t wlo, uint32_t whi) {
    const uint32_t nf = (uint32_t)__popc(fmask);
    return {fmask, nf, n - nf, wlo, whi};
}

// rank of general i among the loyal ones
__device__ __forceinline__ uint32_t round_lrank(const RoundWord& c, uint32_t i) {
    return (uint32_t)__popc(~c.F & ((1u << i) - 1u));
}

// the loyal generals' planes, counted
template <int N>
__device__ __forceinline__ RoundCount round_loyal(const RoundWord& c, const uint64_t (&x)[N]) {
    RoundCount ls;
#pragma unroll
    for (int j = 0; j < N; ++j)
        if (!((c.F >> j) & 1u)) ls.add(x[j]);
    return ls;
}

// `ls` plus what recipient i alone is shown in a one-bit round whose free bits
// start at `base`: mine = i's own true value (i faulty), rl = i's loyal rank
__device__ __forceinline__ RoundCount round_votes(const RoundWord& c, const RoundCount& ls, bool fi,
                                                  uint64_t mine, uint32_t base, uint32_t rl) {
    RoundCount t = ls;
    if (fi) {
        t.add(mine);
    } else {
        for (uint32_t rf = 0; rf < c.nf; ++rf) t.add(enum_plane(base + rf * c.ell + rl, c.wlo, c.whi));
    }
    return t;
}

// The |F| free two-bit proposals to the loyal recipient of rank rl, from `pbase`,
// onto d1 (attack proposed) and d0 (retreat proposed).
__device__ __forceinline__ void round_proposals(const RoundWord& c, RoundCount& d1, RoundCount& d0,
                                                uint32_t pbase, uint32_t rl) {
    for (uint32_t rf = 0; rf < c.nf; ++rf) {
        const uint32_t b = pbase + 2u * (rf * c.ell + rl);
        const uint64_t lo = enum_plane(b, c.wlo, c.whi), hi = enum_plane(b + 1u, c.wlo, c.whi);
        d1.add(lo & hi);   // lo = 1: the proposal is hi
        d0.add(lo & ~hi);  // lo = 0: no proposal, whatever hi is
    }
}

// decisions = the lieutenants' final planes; never undefined
template <int N>
__device__ __forceinline__ void round_decide(const RoundWord& c, const uint64_t (&x)[N], EnumTally<false>& ty) {
#pragma unroll
    for (int r = 1; r < N; ++r) ty.put((uint32_t)(r - 1), !((c.F >> r) & 1u), x[r]);
}

// of(integral_constant<int, n>), n in [1, MAXN]: the kernel instantiated for n generals
template <int MAXN, typename Of>
static auto round_kernel_of(uint32_t n, Of of) {
    if constexpr (MAXN > 1)
        if (n < (uint32_t)MAXN) return round_kernel_of<MAXN - 1>(n, of);
    return of(std::integral_constant<int, MAXN>{});
}

}  // namespace ba
