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
// The tile loop, the counters, the witness and the per-trial outputs are the frame of
// ba_enum_common.hpp; the word evaluator below hands it the lieutenants' planes.
#include "ba_enum_common.hpp"

namespace ba {

constexpr uint32_t kSmenumPad = 8;  // LP is a multiple of it: 8, 16, 24, 32

template <int FORM, int LP>
__global__ __launch_bounds__(kEnumThreads) void k_smenum(SmenumCase g, uint64_t first_trial,
                                                         uint64_t batch,
                                                         uint64_t* __restrict__ decisions,
                                                         uint8_t* __restrict__ outcome,
                                                         uint64_t* __restrict__ counters,
                                                         unsigned long long* __restrict__ witness,
                                                         Sink sk) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smenum_lds[];
    const uint32_t n = g.n, L = n - 1u;
    const uint32_t F = g.fmask;
    const uint32_t lts = (n >= 32u ? 0xFFFFFFFFu : ((1u << n) - 1u)) & ~1u;
    const bool F0 = (F & 1u) != 0;
    const uint32_t nf = (uint32_t)__popc(F), fL = (uint32_t)__popc(F & lts), l = L - fL;
    const uint32_t K = g.me < fL ? g.me : fL;
    const uint32_t two = F0 ? 2u : 1u;                       // bits of one (sender, recipient)
    const uint32_t senders = FORM == 0 ? fL : 1u;            // the coalition sends as one
    const uint32_t per = senders * l * two;                  // bits of one relay round
    const uint32_t rbase = F0 ? 2u * l : 0u;                 // first bit of round 1
    const uint32_t obv = g.order == 1u ? 1u : 0u;
    const uint64_t ob = obv ? ~0ull : 0ull;
    // in-bound is SM's: |F| <= m
    const EnumRun run{n, F, g.order, 0u, nf <= g.m, first_trial, batch, decisions, outcome, counters, witness};
    enum_frame<false, true>(run, smenum_lds, sk, [&](uint32_t wlo, uint32_t whi, EnumTally<false>& ty) {
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
                        for (uint32_t jr = 0; jr < senders; ++jr) {
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
        uint32_t rest = ~F & lts;  // the loyal lieutenants not yet met, in ascending index
#pragma unroll
        for (int lr = 0; lr < LP; ++lr) {
            if ((uint32_t)lr < l) {
                ty.put((uint32_t)__builtin_ctz(rest) - 1u, true, has1[lr] & ~has0[lr]);
                rest &= rest - 1u;
            }
        }
        ty.put_same((F & lts) >> 1, Af);
    });
}

using SmenumKernel = void (*)(SmenumCase, uint64_t, uint64_t, uint64_t*, uint8_t*, uint64_t*,
                              unsigned long long*, Sink);

template <int FORM>
static SmenumKernel smenum_kernel_of(uint32_t l) {
    static constexpr SmenumKernel tab[] = {k_smenum<FORM, 8>, k_smenum<FORM, 16>, k_smenum<FORM, 24>,
                                           k_smenum<FORM, 32>};
    return tab[l <= kSmenumPad ? 0u : (l - 1u) / kSmenumPad];
}

// One persistent launch of enum_geometry's shape (at most 15.5 KiB of decision planes).
// The kernel is picked by the loyal lieutenants' count, padded to a multiple of
// kSmenumPad.
hipError_t launch_smenum(const RunArgs& a, const SmenumCase& g, uint64_t* witness) {
    if (a.n < 1 || a.n > 32 || g.n != a.n || g.form > 1 || a.batch == 0 || g.me > a.n)
        return hipErrorInvalidValue;
    const uint32_t lts = (a.n >= 32u ? 0xFFFFFFFFu : ((1u << a.n) - 1u)) & ~1u;
    if (g.fmask & ~(lts | 1u)) return hipErrorInvalidValue;
    const uint32_t l = a.n - 1u - (uint32_t)__builtin_popcount(g.fmask & lts);
    const EnumGeometry ge = enum_geometry(a, (uint32_t)sizeof(EnumEntry<false>), 0u);
    ProfScope ps(a.prof, "k_smenum", a.stream);
    const SmenumKernel k = g.form == 0 ? smenum_kernel_of<0>(l) : smenum_kernel_of<1>(l);
    hipLaunchKernelGGL(k, dim3(ge.blocks), dim3(ge.threads), ge.lds, a.stream, g, a.first_trial, a.batch,
                       a.decisions, a.outcome, a.counters, (unsigned long long*)witness, a.sink);
    return hipGetLastError();
}

}  // namespace ba
