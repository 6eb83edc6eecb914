// ba_king_common.hpp -- device helpers of the kernels on the King frame alone,
// k_king (ba_king.hip, docs/SEMANTICS.md §9), k_king3 (ba_king3.hip, §10) and k_rand
// (ba_rand.hip, §13): all hold one 64-trial word per wave, lane (i, s) = recipient i
// and sender slice s.  What they share with the other word-per-wave kernels is
// ba_wave_proto.hpp's.
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

// ---------------------------------------------------------------------------
// The all-to-all rounds with one or two tallies from one walk over the sender
// pairs: k_king3's value and propose rounds and k_rand's (ba_rand.hip, §13) report
// and propose rounds.  Wave has the planes F, pref, pa, pr [kMaxN] and
// part[kKing3PartPlanes][64]; TAG is the protocol's Philox tag.
// ---------------------------------------------------------------------------
constexpr int kKing3PartPlanes = 5;   // a slice counts at most 16 messages
using Tally3 = Count<kKing3PartPlanes>;

// a group's count (four digits, up to 8) added into a slice's tally
__device__ __forceinline__ void king3_tally_add(Tally3& tally, const uint64_t (&digit)[4]) {
    uint64_t carry = 0;
#pragma unroll
    for (int p = 0; p < 4; ++p) {
        const uint64_t t = tally.c[p];
        tally.c[p] = xor3(t, digit[p], carry);
        carry = maj3(t, digit[p], carry);
    }
    tally.c[4] ^= carry;
    static_assert(kKing3PartPlanes == 5, "a slice's tally: up to 16 messages");
}

// One group of G sender pairs of a value round (PROP = false) or a propose round
// (PROP = true): this lane's pairs are u = v0 + 2 g + s.  The value round adds the
// 2 G votes general i is shown into t1 (own = its preference plane, read from
// s.pref); the propose round adds the attack proposals it is shown into t1 and the
// retreat proposals into t0 (own1 / own0 = its own proposal planes; the senders'
// are s.pa and s.pr), both from one draw: a faulty sender's coin is its attack
// proposal, the complement its retreat proposal.
template <uint32_t TAG, bool COIN, int G, bool PROP, class Wave>
__device__ __forceinline__ void king3_group(const Wave& s, uint32_t i, uint32_t sl, uint32_t v0,
                                            uint32_t n, uint32_t npairs, uint32_t q, uint64_t gw,
                                            uint64_t seed, uint64_t own1, uint64_t own0, Tally3& t1,
                                            Tally3& t0) {
    const uint32_t odd = i & 1u;
    // Before the draw only what decides it is loaded (the senders' planes come
    // after it: held across the calls they cost registers).
    uint32_t ja[G];
    bool act[G], need = false;
#pragma unroll
    for (int g = 0; g < G; ++g) {
        const uint32_t u = v0 + 2u * (uint32_t)g + sl;  // <= 15: senders 2u, 2u + 1 <= 31
        act[g] = u < npairs;
        ja[g] = 2u * (act[g] ? u : 0u);
        // the lane's own call is sender ja + odd's; it serves recipients i and i ^ 1
        need |= act[g] && s.F[ja[g] + odd] != 0 && (i & ~1u) < n;
    }
    uint64_t ca[G], cb[G];  // what a faulty sender 2u / 2u + 1 shows recipient i
#pragma unroll
    for (int g = 0; g < G; ++g) ca[g] = cb[g] = odd ? ~0ull : 0ull;  // BA_KING_SPLIT: r & 1
    if constexpr (COIN) {
        if (__ballot(need) != 0) {
            const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
            P4 c[G];
#pragma unroll
            for (int g = 0; g < G; ++g)
                c[g] = P4{16u * (ja[g] + odd) + (i >> 1), TAG + q, (uint32_t)gw, (uint32_t)(gw >> 32)};
            if constexpr (G == 1) c[0] = philox10(c[0], k0, k1);
            else philox10_n<G>(c, k0, k1);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                const KingCoin h = king_halves(c[g], odd);
                const uint64_t got = swap_neighbour(h.give);
                ca[g] = odd ? got : h.keep;
                cb[g] = odd ? h.keep : got;
            }
        }
    }
    // the group's 2 G <= 8 messages carry-saved in compile-time order, then the
    // count's four digits added to the tally once
    const uint64_t* src1 = PROP ? s.pa : s.pref;
    Csa<4> v1, v0s;
    static_for_h<0, G>([&](auto gi) {
        constexpr int g = gi();
        // an inactive pair sends nothing; a general counts its own true message
        const uint64_t Fa = s.F[ja[g]], Fb = s.F[ja[g] + 1];
        const bool sa = ja[g] == i, sb = ja[g] + 1 == i;
        uint64_t ma = sa ? own1 : (src1[ja[g]] & ~Fa) | (Fa & ca[g]);
        uint64_t mb = sb ? own1 : (src1[ja[g] + 1] & ~Fb) | (Fb & cb[g]);
        if (!act[g]) ma = mb = 0;
        v1.template add<2 * g>(ma);
        v1.template add<2 * g + 1>(mb);
        if constexpr (PROP) {
            uint64_t ra = sa ? own0 : (s.pr[ja[g]] & ~Fa) | (Fa & ~ca[g]);
            uint64_t rb = sb ? own0 : (s.pr[ja[g] + 1] & ~Fb) | (Fb & ~cb[g]);
            if (!act[g]) ra = rb = 0;
            v0s.template add<2 * g>(ra);
            v0s.template add<2 * g + 1>(rb);
        }
    });
    uint64_t digit[4];
    v1.template resolve<0, 2 * G, false>(digit, 0);
    king3_tally_add(t1, digit);
    if constexpr (PROP) {
        v0s.template resolve<0, 2 * G, false>(digit, 0);
        king3_tally_add(t0, digit);
    }
}

// All sender pairs of one round, in groups of at most G pairs per lane.
template <uint32_t TAG, bool COIN, bool PROP, class Wave>
__device__ __forceinline__ void king3_round(const Wave& s, uint32_t i, uint32_t sl, uint32_t n,
                                            uint32_t npairs, uint32_t q, uint64_t gw, uint64_t seed,
                                            uint64_t own1, uint64_t own0, Tally3& t1, Tally3& t0) {
    for (uint32_t v0 = 0; v0 < npairs; v0 += 8) {
        const uint32_t left = npairs - v0;  // pairs of both slices: groups of ceil(left / 2)
        if (left > 6) king3_group<TAG, COIN, 4, PROP>(s, i, sl, v0, n, npairs, q, gw, seed, own1, own0, t1, t0);
        else if (left > 4) king3_group<TAG, COIN, 3, PROP>(s, i, sl, v0, n, npairs, q, gw, seed, own1, own0, t1, t0);
        else if (left > 2) king3_group<TAG, COIN, 2, PROP>(s, i, sl, v0, n, npairs, q, gw, seed, own1, own0, t1, t0);
        else king3_group<TAG, COIN, 1, PROP>(s, i, sl, v0, n, npairs, q, gw, seed, own1, own0, t1, t0);
    }
}

// The two slices' tallies of general i merged through s.part: six planes, up to 32.
template <class Wave>
__device__ __forceinline__ Count<kKing3PartPlanes + 1> king3_merge(Wave& s, uint32_t lane,
                                                                   const Tally3& tally) {
    wave_sync();  // the previous merge has read part
#pragma unroll
    for (int b = 0; b < kKing3PartPlanes; ++b) s.part[b][lane] = tally.c[b];
    wave_sync();
    Count<kKing3PartPlanes + 1> c;
    uint64_t carry = 0;
#pragma unroll
    for (int b = 0; b < kKing3PartPlanes; ++b) {
        const uint64_t o = s.part[b][lane ^ 32u];
        c.c[b] = xor3(tally.c[b], o, carry);
        carry = maj3(tally.c[b], o, carry);
    }
    c.c[kKing3PartPlanes] = carry;
    return c;
}

}  // namespace ba
