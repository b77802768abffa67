// frame_build.h — device-only primitives shared by rx_kernels.hip (the receive kernels, the TX checksum fill and
// dk_tx_serialize_kernel) and tx_build_kernels.hip (the three TCP emit kernels): the workgroup shape, the checksum
// residue arithmetic, lane_id, gptr, and the code that lays out and stores an Ethernet2 / IPv4 / TCP-or-UDP header
// composed in registers (tx_store_header). Everything has internal linkage: each unit compiles its own copy.
// The frame stream (RegAcc, stream_chunk and its knobs) is not here but in rx_kernels.hip, with every kernel that
// runs it; of the kernels that build frames that is dk_tx_serialize_kernel alone.
// The checksum arithmetic is explained at the top of rx_kernels.hip.
#pragma once

#include <hip/hip_runtime.h>

#include "rx_common.h"

namespace dk {
namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
static_assert(kWaves == (int)kStagedWaves, "the host computes the dynamic tail's boundary with kStagedWaves");

typedef unsigned short us2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ uint32_t hsum2(uint32_t x, uint32_t acc) {  // acc + lo16(x) + hi16(x)
    const us2 one = {1, 1};
    return __builtin_amdgcn_udot2(__builtin_bit_cast(us2, x), one, acc, false);
}
__device__ __forceinline__ uint32_t bswap16(uint32_t x) { return ((x & 0xFFu) << 8) | ((x >> 8) & 0xFFu); }
// x mod 0xFFFF in [0, 0xFFFE].
__device__ __forceinline__ uint32_t mod_ffff(uint32_t x) {
    x = (x & 0xFFFFu) + (x >> 16);
    x = (x & 0xFFFFu) + (x >> 16);
    return x == 0xFFFFu ? 0u : x;
}
// The reference's `!fold(0xFFFF + S)` given m = S mod 0xFFFF (S = sum of BE words incl. pseudo-header).
__device__ __forceinline__ uint32_t csum_from_residue(uint32_t m) { return m == 0 ? 0u : 0xFFFFu - m; }
// BE residue of a LE-half sum.
__device__ __forceinline__ uint32_t be_residue(uint32_t le_sum) { return bswap16(mod_ffff(le_sum)); }

__device__ __forceinline__ uint32_t lane_id() { return __builtin_amdgcn_mbcnt_hi(~0u, __builtin_amdgcn_mbcnt_lo(~0u, 0u)); }

// A global pointer in address space 1: where the compiler cannot prove a parameter's pointer global (TxParams in the
// split TX kernel) it emits flat loads and stores, which count in lgkmcnt too, so every LDS wait after them (the split
// kernels' hand-off spins and releases) also waits for the memory access: a descriptor prefetch or a window rewrite
// then stalls the hand-off for a full memory round trip.
template <class T>
__device__ __forceinline__ __attribute__((address_space(1))) T* gptr(T* p) {
    return (__attribute__((address_space(1))) T*)(p);
}

__device__ __forceinline__ uint32_t be16_sum(uint32_t x) { return (x >> 16) + (x & 0xFFFFu); }  // the BE words of a u32
// BE words of an address held in octet order (dk_rx.h conventions).
__device__ __forceinline__ uint32_t ip_be_sum(uint32_t a) { return bswap16(a & 0xFFFFu) + bswap16(a >> 16); }

// The first hb bytes (42 or 54: Ethernet2 + IPv4 + UDP, or + the fixed TCP header) of a header, given as LE dwords
// d[0 .. 13], stored at a. Even a: a 16-bit head when a is 2 mod 4, then dwords up to the next 16-byte boundary, 16-byte
// stores while four dwords are left, dwords again, and a 16-bit tail when a is 0 mod 4. The common layouts are wide:
// a 16-byte aligned payload behind a 54-byte header puts a at 10 mod 16 (16-bit, dword, three 16-byte stores), a
// 64-byte aligned frame slot puts it at 0 (three 16-byte stores, dword, 16-bit). Odd a: byte stores. Every index into d
// is a compile-time constant (registers, no scratch): one unrolled store sequence per count of leading dwords.
template <int kLead>
__device__ __forceinline__ void tx_store_dwords(uint8_t* base, const uint32_t (&e)[13], uint32_t ndw) {
    typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
    const auto q = gptr(reinterpret_cast<uint32_t*>(base));
#pragma unroll
    for (int k = 0; k < kLead; k++)
        if ((uint32_t)k < ndw) q[k] = e[k];
#pragma unroll
    for (int k = kLead; k < 13; k += 4) {
        if (k + 4 <= 13 && (uint32_t)(k + 4) <= ndw) {
            *gptr(reinterpret_cast<u32x4*>(base + 4 * k)) = u32x4{e[k], e[k + 1 < 13 ? k + 1 : 12],
                                                                    e[k + 2 < 13 ? k + 2 : 12], e[k + 3 < 13 ? k + 3 : 12]};
        } else {
#pragma unroll
            for (int m = k; m < k + 4 && m < 13; m++)
                if ((uint32_t)m < ndw) q[m] = e[m];
        }
    }
}
__device__ __forceinline__ void tx_store_header(uint8_t* a, const uint32_t (&d)[14], bool tcp) {
    const uint32_t am = (uint32_t)reinterpret_cast<uintptr_t>(a);
    const uint32_t ndw = tcp ? 13u : 10u;  // whole dwords between head and tail: (hb - 2) / 4
    if (am & 1u) {
        const auto g = gptr(a);
#pragma unroll
        for (int k = 0; k < 54; k++)
            if (tcp || k < 42) g[k] = (uint8_t)(d[k >> 2] >> ((k & 3) * 8));
        return;
    }
    uint32_t e[13];
    const uint32_t b = am & 2u;  // funnel-shift byte count: 0 or 2
#pragma unroll
    for (int k = 0; k < 13; k++) e[k] = __builtin_amdgcn_alignbyte(d[k + 1], d[k], b);
    if (b) *gptr(reinterpret_cast<uint16_t*>(a)) = (uint16_t)d[0];
    const uint32_t lead = ((0u - (am + b)) & 15u) >> 2;  // dwords up to the next 16-byte boundary
    if (lead == 0) tx_store_dwords<0>(a + b, e, ndw);
    else if (lead == 1) tx_store_dwords<1>(a + b, e, ndw);
    else if (lead == 2) tx_store_dwords<2>(a + b, e, ndw);
    else tx_store_dwords<3>(a + b, e, ndw);
    if (!b) *gptr(reinterpret_cast<uint16_t*>(a + 4 * ndw)) = (uint16_t)(tcp ? d[13] : d[10]);
}

}  // namespace
}  // namespace dk
