// tcp_cc_math.h — the arithmetic rules of dk_tcp.h's congestion-control section, one copy for the device and the
// host: Rust's saturating f32 -> u32 cast, Duration::as_secs_f32, Duration::from_secs_f64 (dk_tcp_rto_ns) and the
// correctly rounded f32 cube root. The including file sets `#pragma clang fp contract(off)` first: every operation
// here is rounded once, in source order. Internal to libdk_rx.so.
#ifndef DK_TCP_CC_MATH_H
#define DK_TCP_CC_MATH_H

#include <cmath>
#include <cstdint>
#include <cstring>

#if defined(__HIPCC__)
#define DK_CC_HD __host__ __device__ __forceinline__
#else
#define DK_CC_HD inline
#endif

namespace dk_cc {

constexpr uint64_t kNsPerSec = 1000000000ull;
constexpr double kMaxRtoSecs = 1e9;

// `x as u32` (Rust): NaN and negatives 0, >= 2^32 saturates, else truncation. The C++ cast is undefined there.
DK_CC_HD uint32_t f32_as_u32(float x) {
    if (!(x > 0.0f)) return 0u;  // NaN, -x, +-0
    if (x >= 4294967296.0f) return 0xFFFFFFFFu;
    return (uint32_t)x;
}

// Duration::as_secs_f32 (core/time.rs): secs as f32 + nanos as f32 / 1e9f.
DK_CC_HD float as_secs_f32(uint64_t ns) {
    const float secs = (float)(ns / kNsPerSec), nanos = (float)(uint32_t)(ns % kNsPerSec);
    const float frac = nanos / 1000000000.0f;
    return secs + frac;
}

DK_CC_HD bool rto_valid(double rto) { return rto >= 0.0 && rto <= kMaxRtoSecs; }

// Duration::from_secs_f64(rto) in nanoseconds: rto * 10^9 rounded to nearest, ties to even, exactly: the 53-bit
// mantissa times 10^9 as a 128-bit integer (hi:lo, from two partial products), shifted right with round and sticky
// bits. rto <= 1e9 < 2^30, so the shift is at least 23 and the result is below 2^60. 0 for an invalid rto.
DK_CC_HD uint64_t rto_ns(double rto) {
    if (!rto_valid(rto)) return 0;
    uint64_t bits;
    memcpy(&bits, &rto, 8);
    const uint32_t ex = (uint32_t)(bits >> 52) & 0x7FFu;
    uint64_t m = bits & 0xFFFFFFFFFFFFFull;
    if (ex) m |= 1ull << 52;
    if (m == 0) return 0;
    // rto = m * 2^(e - 1075), e = max(ex, 1): shift right by s = 1075 - e
    const uint32_t s = 1075u - (ex ? ex : 1u);
    const uint64_t plo = (m & 0xFFFFFFFFull) * kNsPerSec, phi = (m >> 32) * kNsPerSec;  // < 2^62, < 2^51
    const uint64_t lo = plo + (phi << 32);
    const uint64_t hi = (phi >> 32) + (lo < plo ? 1u : 0u);  // < 2^20: the product is below 2^84
    if (s > 84) return 0;  // below a half
    const auto bit = [&](uint32_t k) -> uint64_t { return k < 64 ? (lo >> k) & 1u : (hi >> (k - 64)) & 1u; };
    uint64_t q;
    if (s < 64) q = (hi << (64 - s)) | (lo >> s);  // s >= 23: hi << (64 - s) loses nothing (hi < 2^20, 64 - s <= 41)
    else q = s == 64 ? hi : hi >> (s - 64);
    const uint32_t r = s - 1;  // the round bit's position; sticky = any bit below it
    bool sticky;
    if (r < 64) sticky = (lo & ((1ull << r) - 1)) != 0;
    else sticky = lo != 0 || (r > 64 && (hi & ((1ull << (r - 64)) - 1)) != 0);
    if (bit(r) && (sticky || (q & 1u))) q++;
    return q;
}

// The correctly rounded f32 cube root of a finite x >= 0. The f64 cube root (within an ulp or so of the real value)
// rounded to f32 is right unless the f64 value sits next to the midpoint m of two adjacent f32 values; there the sign
// of x - m^3 decides, exactly: m has 25 significant bits, so m * m is exact in f64 and m^3 = p + e with p = fl(m2 * m),
// e = fma(m2, m, -p); p - x is exact (Sterbenz: p is within a factor 2 of x). x == m^3 cannot happen (m^3 needs 73
// bits).
DK_CC_HD float cbrt_f32(float x) {
    if (!(x > 0.0f) || x == INFINITY) return x;  // 0, NaN, inf
    const double xd = (double)x, r = cbrt(xd);
    const float y = (float)r;
    uint32_t yb;
    memcpy(&yb, &y, 4);
    const uint32_t ob = (double)y <= r ? yb + 1 : yb - 1;  // y's neighbour on r's side
    float other;
    memcpy(&other, &ob, 4);
    const double m = 0.5 * ((double)y + (double)other);
    if (!(fabs(r - m) <= r * 0x1p-46)) return y;
    const double m2 = m * m, p = m2 * m, e = fma(m2, m, -p);
    const double d = (p - xd) + e;  // the sign of m^3 - x
    const float lower = y < other ? y : other, upper = y < other ? other : y;
    return d < 0.0 ? upper : lower;
}

}  // namespace dk_cc

#endif  // DK_TCP_CC_MATH_H
