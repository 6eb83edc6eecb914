// ba_wave_proto.hpp -- what the word-per-wave protocol kernels share: k_sm
// (ba_sm.hip), k_adv (ba_adv.hip), k_king (ba_king.hip), k_king3 (ba_king3.hip),
// k_rand (ba_rand.hip) and k_rstall (ba_rstall.hip); k_enum (ba_enum.hip) and the host take general_mask.  Each holds
// 64-trial words bit-sliced in wave-private LDS planes, takes the trials' inputs
// with lane = trial, and ends a word with lane = trial again: a bit column picked
// out of the planes, trial_result, and the word's counters folded into one lane
// per counter.  (k_rstall keeps lane = trial throughout and takes the prologue and the
// epilogue only.)
#pragma once
#include "ba_engine.hpp"

namespace ba {

// bits 0..n-1: the generals of a faulty mask (n <= 32)
__host__ __device__ __forceinline__ uint32_t general_mask(uint32_t n) {
    return n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u);
}

// orders this wave's LDS accesses for the compiler (no instruction: one wave's
// DS operations complete in order)
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ __forceinline__ void lds_or(uint64_t* p, uint64_t v) {
    (void)__hip_atomic_fetch_or((unsigned long long*)p, (unsigned long long)v, __ATOMIC_RELAXED,
                                __HIP_MEMORY_SCOPE_WORKGROUP);
}

// Prologue, lane = trial i of the call: the trial's faulty mask and order code,
// loaded where they are given, drawn where GEN says some are generated (gen_trial
// leaves a given one alone), the mask cut to the n generals (all =
// general_mask(n)).  A trial past the batch: nobody faulty, retreat.
template <bool GEN>
__device__ __forceinline__ void trial_inputs(bool live, uint32_t n, uint32_t all, uint64_t seed,
                                             const GenSpec& gen, uint64_t first_trial, uint64_t i,
                                             const uint32_t* __restrict__ faulty,
                                             const uint8_t* __restrict__ order, uint32_t& fm,
                                             uint32_t& oc) {
    fm = 0, oc = 0;
    if (live) {
        if (gen.faulty_mode == 0) fm = faulty[i];
        if (gen.order_mode == 0) oc = order[i];
        if constexpr (GEN) gen_trial(n, seed, gen, first_trial + i, fm, oc);
    }
    fm &= all;
}

// The word's faulty plane of general g: a ballot over the trials' masks.
__device__ __forceinline__ uint64_t faulty_plane(uint32_t fm, uint32_t g) {
    return __ballot(((fm >> g) & 1u) != 0);
}

// Epilogue, lane = trial b: bit b of one 64-bit LDS plane (one 32-bit read); the
// caller's loop over its planes gathers the lane's bit column.  (k_adv and k_enum
// read two interleaved columns of 16-byte pairs with one index expression and keep
// that form: through this helper their instruction streams changed.)
__device__ __forceinline__ uint32_t lane_bit(const void* plane, uint32_t lane) {
    return (reinterpret_cast<const uint32_t*>(plane)[lane >> 5] >> (lane & 31u)) & 1u;
}

// Wave totals of one word's run counters added into `mine` (lane c holds
// counter c): flags by ballot + popcount, the small integers bit-sliced
// (faulty_total up to 32 per trial: six planes).  UNDEF: the protocol has
// undefined decisions to count (r.nU).
template <bool UNDEF>
__device__ __forceinline__ void lane_counts_add(bool live, const TrialResult& r, uint32_t lane,
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
        if constexpr (UNDEF) c[C_UNDEF] += (uint32_t)__popcll(__ballot(live && ((r.nU >> b) & 1u))) << b;
        c[C_FTOT] += (uint32_t)__popcll(__ballot(live && ((r.nf >> b) & 1u))) << b;
        c[C_ATT] += (uint32_t)__popcll(__ballot(live && ((r.nA >> b) & 1u))) << b;
    }
#pragma unroll
    for (int i = 0; i < C_NUM; ++i)
        if (lane == (uint32_t)i) mine += c[i];
}

}  // namespace ba
