// ba_bitslice.hpp -- 8x8 bit-matrix helpers behind k_om3wt's byte-sliced input
// staging and result pick-out (ba_wave.hpp).  A lane that owns 8 consecutive
// trials of one 64-trial word converts between "one value per trial" and "byte
// k of every bit plane" with a few 8x8 bit transposes in registers, where the
// ballot staging and the bfe pick-out moved one bit at a time.
// Everything here is __host__ __device__ with the same results on both sides
// (tests/native/byte_slice_check.cpp runs it on the host against the per-trial
// definitions); only byte_perm has a device form of its own (v_perm_b32).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>

namespace ba {

// An 8x8 bit matrix: row r is byte r (rows 0-3 in lo, 4-7 in hi), column c is
// bit c of the byte.
struct Bits8x8 {
    uint32_t lo, hi;
};

// v_perm_b32: byte i of the result is byte sel[i] of the 8 bytes {hi, lo}
// (0-3: lo, 4-7: hi), or 0x00 for sel[i] = 0x0c.  sel is a constant.
constexpr uint32_t kPermZero = 0x0c;
__host__ __device__ __forceinline__ uint32_t byte_perm(uint32_t hi, uint32_t lo, uint32_t sel) {
#ifdef __HIP_DEVICE_COMPILE__
    return __builtin_amdgcn_perm(hi, lo, sel);
#else
    const uint64_t src = (uint64_t)hi << 32 | lo;
    uint32_t r = 0;
    for (int i = 0; i < 4; ++i) {
        const uint32_t s = (sel >> (8 * i)) & 0xffu;
        const uint32_t b = s == kPermZero ? 0u : (uint32_t)(src >> (8 * (s & 7u))) & 0xffu;
        r |= b << (8 * i);
    }
    return r;
#endif
}

// Byte 0 of b0..b3 as bytes 0..3 of one dword (whatever the upper bytes hold).
__host__ __device__ __forceinline__ uint32_t pack_bytes4(uint32_t b0, uint32_t b1, uint32_t b2,
                                                         uint32_t b3) {
    return byte_perm(byte_perm(b3, b2, 0x0c0c0400u), byte_perm(b1, b0, 0x0c0c0400u), 0x05040100u);
}
// The same with b1 = b3 = 0: one permute.
__host__ __device__ __forceinline__ uint32_t pack_bytes_even(uint32_t b0, uint32_t b2) {
    return byte_perm(b2, b0, 0x0c040c00u);
}
// Byte B of d0..d3 as bytes 0..3 of one dword.
template <int B>
__host__ __device__ __forceinline__ uint32_t gather_byte(uint32_t d0, uint32_t d1, uint32_t d2,
                                                         uint32_t d3) {
    constexpr uint32_t s = 0x0c0c0000u | (uint32_t)(4 + B) << 8 | (uint32_t)B;
    return byte_perm(byte_perm(d3, d2, s), byte_perm(d1, d0, s), 0x05040100u);
}

// The transpose: bit c of byte r <-> bit r of byte c.  Three swap steps (2x2
// bits, 2x2 blocks of 2x2, 2x2 blocks of 4x4); the first two stay inside a
// 32-bit half, the last exchanges nibbles between the halves.  Each step is
// two shifts and two masked merges per half (v_bfi / v_bitop3 on the device).
__host__ __device__ __forceinline__ uint32_t swap_step(uint32_t x, uint32_t m, int s) {
    return (x & ~(m | m << s)) | ((x & m) << s) | ((x >> s) & m);
}
__host__ __device__ __forceinline__ Bits8x8 transpose8x8(Bits8x8 x) {
    x.lo = swap_step(swap_step(x.lo, 0x00AA00AAu, 7), 0x0000CCCCu, 14);
    x.hi = swap_step(swap_step(x.hi, 0x00AA00AAu, 7), 0x0000CCCCu, 14);
    return Bits8x8{(x.lo & 0x0F0F0F0Fu) | ((x.hi << 4) & 0xF0F0F0F0u),
                   (x.hi & 0xF0F0F0F0u) | ((x.lo >> 4) & 0x0F0F0F0Fu)};
}
__host__ __device__ __forceinline__ uint64_t transpose8x8(uint64_t x) {
    const Bits8x8 t = transpose8x8(Bits8x8{(uint32_t)x, (uint32_t)(x >> 32)});
    return (uint64_t)t.hi << 32 | t.lo;
}

// ---------------------------------------------------------------------------
// Staged inputs of the 8 consecutive trials i0 .. i0+7 (i0 a multiple of 8).
// ---------------------------------------------------------------------------
// The lane's 8 faulty masks and 8 order bytes (o: byte t = trial t).  A lane
// whose trials are all inside [0, batch) takes them with wide loads (only the
// element alignment of the buffers is assumed: the copies are memcpy); any
// other lane loads trial by trial, each load guarded, and leaves 0 for the
// trials at or beyond batch.  nv = the number of its trials inside the batch.
// Nothing outside [0, batch) of either buffer is touched.  base <= batch.
// wide accesses at the element alignment of the C ABI's buffers
typedef uint32_t U32x4 __attribute__((ext_vector_type(4), aligned(4)));  // 4 faulty masks
typedef uint32_t U32x2 __attribute__((ext_vector_type(2), aligned(1)));  // 8 order / outcome bytes
typedef uint64_t U64x2 __attribute__((ext_vector_type(2), aligned(8)));  // 2 decision words
struct StageRaw {
    uint32_t f[8];
    uint32_t o_lo, o_hi;
    uint32_t nv;
};
__host__ __device__ __forceinline__ StageRaw stage_load(const uint32_t* __restrict__ faulty,
                                                        const uint8_t* __restrict__ order,
                                                        uint64_t base, uint32_t off,
                                                        uint64_t batch) {
    // i0 = base + off: base is the wave's first trial (uniform), off the lane's
    // offset from it (a multiple of 8, below 2^30), so the lane's share of the
    // count is 32-bit arithmetic on the uniform remainder
    const uint64_t i0 = base + off;
    // (base <= batch is the caller's; != 0 rather than an ordered 64-bit compare,
    // which the scalar unit lacks)
    const uint64_t rem64 = batch - base;
    const uint32_t rem = (rem64 >> 30) != 0 ? 1u << 30 : (uint32_t)rem64;
    StageRaw r;
    r.nv = rem <= off ? 0u : (rem - off >= 8 ? 8u : rem - off);
    if (r.nv == 8) {
        const U32x4 f0 = *reinterpret_cast<const U32x4*>(faulty + i0),
                    f1 = *reinterpret_cast<const U32x4*>(faulty + i0 + 4);
        const U32x2 o = *reinterpret_cast<const U32x2*>(order + i0);
        r.f[0] = f0.x, r.f[1] = f0.y, r.f[2] = f0.z, r.f[3] = f0.w;
        r.f[4] = f1.x, r.f[5] = f1.y, r.f[6] = f1.z, r.f[7] = f1.w;
        r.o_lo = o.x;
        r.o_hi = o.y;
    } else {
        // rare (the batch's last lanes): one small loop, the values shifted in
        // from the top so that no register is indexed
        for (int t = 0; t < 8; ++t) r.f[t] = 0;
        r.o_lo = r.o_hi = 0;
#pragma clang loop unroll(disable)
        for (uint32_t t = 0; t < 8; ++t) {
            uint32_t fm = 0, c = 0;
            if (t < r.nv) {
                fm = faulty[i0 + t];
                c = order[i0 + t];
            }
            for (int k = 0; k < 7; ++k) r.f[k] = r.f[k + 1];
            r.f[7] = fm;
            r.o_lo = r.o_lo >> 8 | r.o_hi << 24;
            r.o_hi = r.o_hi >> 8 | c << 24;
        }
    }
    return r;
}

// Byte k (this lane's 8 trials, bit t = trial t) of the N+3 input planes of
// the word: F[0..N), OB (order byte == 1), OO (order byte == 2), VAL.  Only the
// low N bits of a faulty mask count.  Two transposes: the masks' bits 0-7, then
// a matrix whose row t holds the mask's bits 8..N-1, the order byte's bits 0-1
// and "one of its bits 2-7 is set" -- OB and OO are one three-input operation
// each on the transposed rows.
template <int N>
struct StagePlanes {
    static_assert(N >= 9 && N <= 13, "mask bits 8..N-1 and three order bits share one matrix");
    Bits8x8 f07;  // byte g: plane F[g], g < 8
    Bits8x8 hi;   // bytes 0..N-9: F[8..N); then OB, OO
    uint32_t val;
    template <int G>
    __host__ __device__ __forceinline__ uint32_t plane() const {
        if constexpr (G < 4) return (f07.lo >> (8 * G)) & 0xffu;
        else if constexpr (G < 8) return (f07.hi >> (8 * (G - 4))) & 0xffu;
        else if constexpr (G == N + 2) return val;
        else if constexpr (G - 8 < 4) return (hi.lo >> (8 * (G - 8))) & 0xffu;
        else return (hi.hi >> (8 * (G - 12))) & 0xffu;
    }
};
template <int N>
__host__ __device__ __forceinline__ StagePlanes<N> stage_pack(const StageRaw& r) {
    constexpr int NH = N - 8;  // mask bits in the second matrix
    constexpr uint32_t HM = ((1u << NH) - 1u) * 0x01010101u;
    StagePlanes<N> p;
    p.f07 = transpose8x8(Bits8x8{gather_byte<0>(r.f[0], r.f[1], r.f[2], r.f[3]),
                                 gather_byte<0>(r.f[4], r.f[5], r.f[6], r.f[7])});
    // per byte of o: bit 7 of nz = (o & 0xfc) != 0 (the add carries into bit 7
    // exactly when bits 2-6 are not all clear, and never out of the byte)
    auto row = [&](uint32_t fb1, uint32_t o) -> uint32_t {
        const uint32_t nz = ((o & 0x7C7C7C7Cu) + 0x7F7F7F7Fu) | o;
        return (fb1 & HM) | ((o & 0x03030303u) << NH) | ((nz >> (5 - NH)) & (0x04040404u << NH));
    };
    const Bits8x8 t = transpose8x8(Bits8x8{row(gather_byte<1>(r.f[0], r.f[1], r.f[2], r.f[3]), r.o_lo),
                                           row(gather_byte<1>(r.f[4], r.f[5], r.f[6], r.f[7]), r.o_hi)});
    // rows of t: 0..NH-1 = F[8..N), NH = order bit 0, NH+1 = order bit 1, NH+2 = nz
    const uint64_t t64 = (uint64_t)t.hi << 32 | t.lo;
    const uint32_t o0 = (uint32_t)(t64 >> (8 * NH)) & 0xffu, o1 = (uint32_t)(t64 >> (8 * NH + 8)) & 0xffu,
                   nz = (uint32_t)(t64 >> (8 * NH + 16)) & 0xffu;
    const uint32_t ob = o0 & ~o1 & ~nz, oo = o1 & ~o0 & ~nz;
    const uint64_t h = (t64 & ((1ull << (8 * NH)) - 1ull)) | (uint64_t)ob << (8 * NH) |
                       (uint64_t)oo << (8 * NH + 8);
    p.hi = Bits8x8{(uint32_t)h, (uint32_t)(h >> 32)};
    p.val = (1u << r.nv) - 1u;
    return p;
}

// ---------------------------------------------------------------------------
// Pick-out: the lane's 8 trials' decision words and outcome bytes from byte k
// of the root planes a[b] = A[b], u[b] = U[b] (b < L; u is read only for even
// L, an odd L never ties) and of the six outcome planes o[0..6).  Only byte 0
// of every input counts.  dec[t]: bit 2b = A[b], bit 2b+1 = U[b] of trial t;
// byte t of (out_hi, out_lo) = the outcome byte of trial t.
// Lieutenants 4j..4j+3 fill one matrix (A on even rows, U on odd ones) whose
// transposed byte t is byte j of dec[t]; the outcome planes are rows 0-5 of a
// last matrix, and when one lieutenant is left over (L % 4 == 1, as for L = 9)
// it rides on that matrix's rows 6-7 instead of taking a matrix of its own.
// ---------------------------------------------------------------------------
template <int L>
struct PickOut {
    static_assert(L >= 1 && L <= 16, "decision word: 2 bits per lieutenant in 32 bits");
    static constexpr bool TIES = L % 2 == 0, SHARE = L % 4 == 1;
    static constexpr int ND = SHARE ? L / 4 : (L + 3) / 4;  // decision matrices
    uint32_t dec[8];
    uint32_t out_lo, out_hi;
};
template <int L>
__host__ __device__ __forceinline__ PickOut<L> pick_out(const uint32_t (&a)[L], const uint32_t (&u)[L],
                                                        const uint32_t (&o)[6]) {
    using P = PickOut<L>;
    constexpr int ND = P::ND;
    auto A = [&](int b) -> uint32_t { return b < L ? a[b] : 0u; };
    auto U = [&](int b) -> uint32_t { return b < L ? u[b] : 0u; };
    Bits8x8 m[ND > 0 ? ND : 1];
#pragma unroll
    for (int j = 0; j < ND; ++j) {
        Bits8x8 x;
        if constexpr (P::TIES) {
            x.lo = pack_bytes4(A(4 * j), U(4 * j), A(4 * j + 1), U(4 * j + 1));
            x.hi = pack_bytes4(A(4 * j + 2), U(4 * j + 2), A(4 * j + 3), U(4 * j + 3));
        } else {
            x.lo = pack_bytes_even(A(4 * j), A(4 * j + 1));
            x.hi = pack_bytes_even(A(4 * j + 2), A(4 * j + 3));
        }
        m[j] = transpose8x8(x);
    }
    Bits8x8 x;
    x.lo = pack_bytes4(o[0], o[1], o[2], o[3]);
    if constexpr (!P::SHARE) x.hi = byte_perm(o[5], o[4], 0x0c0c0400u);
    else if constexpr (P::TIES) x.hi = pack_bytes4(o[4], o[5], a[L - 1], u[L - 1]);
    else x.hi = byte_perm(a[L - 1], byte_perm(o[5], o[4], 0x0c0c0400u), 0x0c040100u);
    const Bits8x8 mo = transpose8x8(x);
    P r;
    r.out_lo = mo.lo & 0x3F3F3F3Fu;
    r.out_hi = mo.hi & 0x3F3F3F3Fu;
#pragma unroll
    for (int t = 0; t < 8; ++t) {
        const uint32_t bt = (uint32_t)t & 3u;
        auto half = [&](const Bits8x8& b) -> uint32_t { return t < 4 ? b.lo : b.hi; };
        uint32_t d = 0;
        if constexpr (ND >= 2) d = byte_perm(half(m[1]), half(m[0]), 0x0c0c0000u | (4 + bt) << 8 | bt);
        else if constexpr (ND == 1) d = byte_perm(0u, half(m[0]), 0x0c0c0c00u | bt);
        if constexpr (ND >= 4)
            d |= byte_perm(half(m[3]), half(m[2]), 0x00000c0cu | (4 + bt) << 24 | bt << 16);
        else if constexpr (ND == 3) d |= byte_perm(0u, half(m[2]), 0x0c000c0cu | bt << 16);
        if constexpr (P::SHARE)
            d |= ((half(mo) >> (8 * bt + 6)) & (P::TIES ? 3u : 1u)) << (8 * ND);
        r.dec[t] = d;
    }
    return r;
}

}  // namespace ba
