// ba_om3_task.hpp -- per-task helpers of k_om3wt outside its rounds (ba_wave.hpp):
// the lane's two byte tables in closed form and the root majorities in 32-bit
// halves.  Everything here is __host__ __device__ with the same results on both
// sides; tests/native/om3_task_check.cpp runs it on the host against the
// definitions it replaces (Om3LaneOffsets' lambdas, roots_r1t).
#pragma once
#include "ba_device.hpp"

namespace ba {

// a * b for a, b < 2^24 (v_mul_u32_u24: full rate, where v_mul_lo_u32 is quarter rate)
__host__ __device__ __forceinline__ uint32_t mul_u24(uint32_t a, uint32_t b) {
#ifdef __HIP_DEVICE_COMPILE__
    return __umul24(a, b);
#else
    return a * b;
#endif
}
// p advanced by a byte offset
template <typename T>
__host__ __device__ __forceinline__ T* lds_at(T* p, uint32_t bytes) {
    using B = std::conditional_t<std::is_const<T>::value, const char, char>;
    return reinterpret_cast<T*>(reinterpret_cast<B*>(p) + bytes);
}

// The byte tables of Om3LaneOffsets (ba_wave.hpp) for S <= 7 members, as one
// 64-bit word each:
//   mem byte a = 8 (a + (a >= la))      r2t byte d = 8 CP (d >= la)
// Both are a constant plus a constant under the mask of the bytes a >= la, which
// is one shift of la (la <= S: the shift stays below 64).  No byte carries
// (8 S and 8 CP are below 256), so the sum is taken per 32-bit half.  Against
// the 2 S compares, selects and ors of the per-byte definition: 8 instructions.
struct Om3LaneTables {
    uint64_t mem, r2t;
};
constexpr uint64_t bytes_of(int count, uint32_t v, uint32_t step) {
    uint64_t r = 0;
    for (int a = 0; a < count; ++a) r |= (uint64_t)((v + step * a) & 0xffu) << (8 * a);
    return r;
}
template <int S, int CP>
__host__ __device__ __forceinline__ Om3LaneTables om3_lane_tables(uint32_t la) {
    static_assert(S >= 1 && S <= 7 && 8 * S < 256 && 8 * CP < 256, "one byte per member, la <= S");
    constexpr uint64_t ramp = bytes_of(S, 0, 8), step = bytes_of(S, 8, 0), row = bytes_of(S, 8 * CP, 0);
    const uint64_t keep = ~0ull << (8 * la);
    const uint32_t klo = (uint32_t)keep, khi = (uint32_t)(keep >> 32);
    const uint32_t mlo = (uint32_t)ramp + ((uint32_t)step & klo);
    const uint32_t mhi = (uint32_t)(ramp >> 32) + ((uint32_t)(step >> 32) & khi);
    return Om3LaneTables{(uint64_t)mhi << 32 | mlo, row & keep};
}

// Root majorities of W words from R1T in 32-bit halves (L odd: no ties, so only
// the A plane exists).  The W L root columns are 2 W L half-columns of L inputs
// each; unit h = 2 (w L + col) + half is the 32-bit half `half` of column col of
// word w.  Trip t gives lane `lane` the unit 64 t + lane: a column is LP words, so
// the unit's inputs are at r1t + 8 LP (h >> 1) + 4 (h & 1) + 8 j bytes and a trip
// moves every lane by the constant 256 LP bytes; the majority goes to the dense
// image a[w L + col], i.e. byte 4 h: +256 per trip.  One address pair per lane
// serves all trips, and a carry-save count of 32-bit values is half the
// instructions of the 64-bit one: 2 W L / 64 trips of 32-bit work, rounded up,
// where lane = column took W L / 64 trips of 64-bit work, rounded up (n = 10:
// three 18-instruction counts instead of two of 36).
template <int L, int W, int LP>
struct Om3RootHalves {
    static_assert(L % 2 == 1, "dense A image: an even L also has a U plane");
    static constexpr uint32_t UNITS = 2 * W * L, TRIPS = (UNITS + 63) / 64;
    static constexpr uint32_t SRC_TRIP = 256 * LP, DST_TRIP = 256;
    __host__ __device__ static __forceinline__ uint32_t src(uint32_t lane) {
        return mul_u24(lane >> 1, 8u * LP) + (lane & 1u) * 4u;
    }
    __host__ __device__ static __forceinline__ uint32_t dst(uint32_t lane) { return 4u * lane; }
    // lanes of trip T that hold a unit
    template <uint32_t T>
    __host__ __device__ static __forceinline__ bool live(uint32_t lane) {
        return 64u * T + lane < UNITS;
    }
    // one unit: in = the L inputs' first dword, 8 bytes apart
    __host__ __device__ static __forceinline__ uint32_t majority(const uint32_t* in) {
        Csa<4, uint32_t> cnt;
        static_assert(L < 16, "four count levels");
        static_for_h<0, L>([&](auto j) { cnt.template add<j()>(in[2 * j()]); });
        return cnt.template ge<L, L / 2 + 1>();
    }
    __host__ __device__ static __forceinline__ void run(const uint64_t* r1t, uint64_t* a,
                                                        uint32_t lane) {
        const char* s = reinterpret_cast<const char*>(r1t) + src(lane);
        char* d = reinterpret_cast<char*>(a) + dst(lane);
        static_for_h<0, (int)TRIPS>([&](auto t) {
            constexpr uint32_t T = (uint32_t)t();
            // (a trip wholly inside the units needs no guard: the wave has 64 lanes)
            if (64u * (T + 1) <= UNITS || live<T>(lane))
                *reinterpret_cast<uint32_t*>(d + T * DST_TRIP) =
                    majority(reinterpret_cast<const uint32_t*>(s + T * SRC_TRIP));
        });
    }
};

}  // namespace ba
