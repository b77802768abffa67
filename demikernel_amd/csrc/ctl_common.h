// ctl_common.h — what the kernel files share beyond rx_common.h: the control-plane families (tcp_listen, tcp_connect,
// tcp_close, arp) all of it, the TCP data-plane contexts (tcp_kernels, tcp_tx, tcp_ack, tcp_ackemit, tcp_cc, tcp_commit)
// the call scaffold of (b).
//   (a) No HIP needed (DK_HD): the checksum helpers, the ISN generator's CRC and the one builder of a TCP frame with no
//       payload. tests/host_asan compiles this part with a host compiler under ASan + UBSan.
//   (b) HIP only: the agent-scope atomic wrappers, scratch carving, the launch grid, the device guard, and the call
//       scaffold: CallOrder, the event that serialises an owner's calls on one device; Buf<T>, a device buffer that
//       waits for that order before it frees; CallScratch, the two together for an owner with one byte scratch.
#pragma once
#include <stddef.h>
#include <stdint.h>
#if defined(__HIPCC__)
#include <errno.h>

#include <algorithm>
#endif

#include "rx_common.h"

namespace dk {
namespace ctl {

// ---- (a) ----------------------------------------------------------------------------------------------------------------
constexpr uint32_t kTcpFrameBytes = 54, kTcpOptFrameBytes = 62;  // Ethernet2 + IPv4 + TCP; with [MSS, WindowScale]
static_assert(DK_TCP_LSN_RST_BYTES == kTcpFrameBytes && DK_TCP_LSN_SYNACK_BYTES == kTcpOptFrameBytes &&
                  DK_TCP_CON_ACK_BYTES == kTcpFrameBytes && DK_TCP_CON_SYN_BYTES == kTcpOptFrameBytes &&
                  DK_TCP_CLS_ACK_BYTES == kTcpFrameBytes,
              "the frame lengths of dk_tcp.h are tcp_frame's");

DK_HD uint32_t be16s(uint32_t x) { return (x >> 16) + (x & 0xFFFFu); }
DK_HD uint32_t bsw16(uint32_t x) { return ((x & 0xFFu) << 8) | ((x >> 8) & 0xFFu); }
DK_HD uint32_t ipbe(uint32_t a) { return bsw16(a & 0xFFFFu) + bsw16(a >> 16); }
DK_HD uint32_t csum_fold(uint32_t s) {
    s = (s >> 16) + (s & 0xFFFFu);
    s = (s >> 16) + (s & 0xFFFFu);
    return ~s & 0xFFFFu;
}

// CRC-32/CKSUM of the 16 bytes isn_generator.rs feeds it (ips in octet order: their first octet is the low byte).
DK_HD uint32_t isn_crc(uint32_t rip, uint32_t rport, uint32_t lip, uint32_t lport, uint32_t nonce) {
    const uint32_t w[4] = {__builtin_bswap32(rip), (rport & 0xFFFFu) << 16 | (__builtin_bswap32(lip) >> 16),
                           (__builtin_bswap32(lip) << 16) | (lport & 0xFFFFu), nonce};
    uint32_t crc = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
        crc ^= w[k];  // four message bytes, most significant first
        for (int b = 0; b < 32; b++) crc = (crc << 1) ^ ((crc >> 31) ? 0x04C11DB7u : 0u);
    }
    return ~crc;
}

// One frame at a: Ethernet2 + IPv4 + TCP with no payload, the bytes dk_tx_serialize writes for the descriptor.
// opts: options [MSS(mss), WindowScale(ws)], 62 bytes; else 54 (mss and ws are not read). A caller that passes a
// constant for opts gets that form alone. A 4-byte aligned a takes dword stores and one 16-bit store, any other byte
// stores.
DK_HD void tcp_frame(uint8_t* a, const dk_tx_link* lk, uint32_t ipw, uint32_t src, uint32_t dst, uint32_t sport,
                     uint32_t dport, uint32_t seq, uint32_t ack, uint32_t b13, uint32_t win, bool opts, uint32_t mss,
                     uint32_t ws, bool offload) {
    const uint32_t* lw = reinterpret_cast<const uint32_t*>(lk);
    const uint32_t hl = opts ? 28u : 20u, tot = 20u + hl;
    const uint32_t ident = ipw & 0xFFFFu, ttl = (ipw >> 16) & 0xFFu, tos = ipw >> 24;
    const uint32_t ipc = csum_fold((0x4500u | tos) + tot + ident + 0x4000u + ((ttl << 8) | 6u) + ipbe(src) + ipbe(dst));
    const uint32_t b12 = (hl / 4) << 4;
    uint32_t c = 0;
    if (!offload) {
        uint32_t s = ipbe(src) + ipbe(dst) + 6u + hl + sport + dport + be16s(seq) + be16s(ack) + ((b12 << 8) | b13) + win;
        if (opts) s += 0x0204u + (mss & 0xFFFFu) + 0x0303u + ((ws & 0xFFu) << 8);
        c = csum_fold(s);
    }
    uint32_t d[16];
    d[0] = lw[0];
    d[1] = lw[1];
    d[2] = lw[2];
    d[3] = 0x0008u | 0x45u << 16 | tos << 24;
    d[4] = bsw16(tot) | bsw16(ident) << 16;
    d[5] = 0x0040u | ttl << 16 | 6u << 24;
    d[6] = bsw16(ipc) | (src & 0xFFFFu) << 16;
    d[7] = (src >> 16) | (dst & 0xFFFFu) << 16;
    d[8] = (dst >> 16) | bsw16(sport) << 16;
    const uint32_t sq = __builtin_bswap32(seq), ak = __builtin_bswap32(ack);
    d[9] = bsw16(dport) | sq << 16;
    d[10] = (sq >> 16) | ak << 16;
    d[11] = (ak >> 16) | b12 << 16 | b13 << 24;
    d[12] = bsw16(win) | bsw16(c) << 16;
    d[13] = opts ? 0x0402u << 16 : 0u;             // urgent pointer 0; kind 2, length 4
    d[14] = bsw16(mss & 0xFFFFu) | 0x0303u << 16;  // the MSS; kind 3, length 3
    d[15] = ws & 0xFFu;                            // the shift; EndOfOptionsList
    const uint32_t nb = opts ? kTcpOptFrameBytes : kTcpFrameBytes;
    if ((reinterpret_cast<uintptr_t>(a) & 3u) == 0) {
        uint32_t* q = reinterpret_cast<uint32_t*>(a);
#pragma unroll
        for (int k = 0; k < 15; k++)
            if ((uint32_t)(4 * k + 4) <= nb) q[k] = d[k];
        if (opts) *reinterpret_cast<uint16_t*>(a + 60) = (uint16_t)d[15];
        else *reinterpret_cast<uint16_t*>(a + 52) = (uint16_t)d[13];
    } else {
#pragma unroll
        for (int k = 0; k < 62; k++)
            if ((uint32_t)k < nb) a[k] = (uint8_t)(d[k >> 2] >> ((k & 3) * 8));
    }
}

#if defined(__HIPCC__)
// ---- (b) ----------------------------------------------------------------------------------------------------------------
constexpr uint32_t kBlock = 256, kWave = 64;
constexpr int kMaxDevices = 64;

__device__ __forceinline__ void min32(uint32_t* p, uint32_t v) {
    __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void max32(uint32_t* p, uint32_t v) {
    __hip_atomic_fetch_max(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ uint32_t add32(uint32_t* p, uint32_t v) {
    return __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void add64(uint64_t* p, uint64_t v) {
    __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

inline size_t round16(size_t b) { return (b + 15) & ~(size_t)15; }

struct Carver {
    uint8_t* b;
    template <class T>
    T* take(size_t count) {
        T* p = reinterpret_cast<T*>(b);
        b += round16(count * sizeof(T));
        return p;
    }
};

// One thread per item, one workgroup at least: a kernel that also writes the call's totals runs for zero items.
inline dim3 grid_for(uint32_t items) { return dim3((std::max(items, 1u) + kBlock - 1) / kBlock); }

struct DeviceGuard {
    int prev = -1;
    explicit DeviceGuard(int dev) {
        if (hipGetDevice(&prev) != hipSuccess) prev = -1;
        if (prev != dev) (void)hipSetDevice(dev);
    }
    ~DeviceGuard() {
        if (prev >= 0) (void)hipSetDevice(prev);
    }
};

// CallOrder, Buf and free_all are internal to the kernel files: hidden, so their inline and template instances are no
// part of the library's symbol list.
#pragma GCC visibility push(hidden)

// The order of an owner's calls (a context's, a table's, a pool entry's) on one device: each call's stream is put behind
// the call before it, so two streams never overlap on the owner's buffers. `last` is the owner's to create, before the
// first record().
struct CallOrder {
    hipEvent_t last = nullptr;
    hipStream_t last_stream = nullptr;
    bool used = false;

    // Stream s ordered behind the last call.
    int order(hipStream_t s) {
        return used && last_stream != s && hipStreamWaitEvent(s, last, 0) != hipSuccess ? EIO : 0;
    }
    // The call's work is queued on s: a launch error surfaces here, and the next call waits for this one.
    int record(hipStream_t s) {
        if (hipGetLastError() != hipSuccess) return EIO;
        if (hipEventRecord(last, s) != hipSuccess) return EIO;
        last_stream = s;
        used = true;
        return 0;
    }
    // The host waits for the last call, if there was one: before a buffer is freed, a table is read, the owner destroyed.
    int drain() { return used && hipEventSynchronize(last) != hipSuccess ? EIO : 0; }
};

// A device buffer of `cap` elements that only grows. Every buffer it frees was waited for: no list of the buffers a
// call is about to grow has to be kept in step with the calls that use them. A first allocation frees nothing and
// waits for nothing.
template <class T>
struct Buf {
    T* p = nullptr;
    size_t cap = 0;

    // At least n elements; drains `o` before the old ones go. EIO, ENOMEM.
    int grow(CallOrder& o, size_t n) {
        if (cap >= n) return 0;
        if (p && o.drain()) return EIO;
        free();
        if (hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(T)) != hipSuccess) return ENOMEM;
        cap = n;
        return 0;
    }
    void free() {
        if (p) (void)hipFree(p);
        p = nullptr, cap = 0;
    }
};

template <class... B>
void free_all(B&... b) {
    (b.free(), ...);
}

#pragma GCC visibility pop

// An owner with one byte scratch, carved anew by every call (Carver).
struct CallScratch : CallOrder {
    Buf<uint8_t> scratch;
    int grow(size_t need) { return scratch.grow(*this, need); }
};

// For the families that keep no table: the current device's entry of `pools` (its event made on first use) with at
// least `need` bytes, the caller's stream ordered behind the entry's last call.
inline int enter_pool(CallScratch (&pools)[kMaxDevices], size_t need, hipStream_t s, CallScratch** out) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= kMaxDevices) return EIO;
    CallScratch* p = &pools[dev];
    if (!p->last && hipEventCreateWithFlags(&p->last, hipEventDisableTiming) != hipSuccess) return EIO;
    if (int rc = p->grow(need)) return rc;
    if (p->order(s)) return EIO;
    *out = p;
    return 0;
}
#endif  // __HIPCC__

}  // namespace ctl
}  // namespace dk
