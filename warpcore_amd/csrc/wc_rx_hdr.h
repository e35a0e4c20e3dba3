// wc_rx_hdr.h -- the Ethernet / IP header view of one frame, shared by the RX
// verdict kernel (wc_k_rx.hip) and the TX seal kernel (wc_k_tx.hip): the
// per-frame header chunk loads that stay inside the frame, and the fields both
// decision chains read (EtherType, version, IHL, lengths, fragment offset,
// protocol / next header).  DESIGN.md sections 8 and 4.7.
#pragma once

#include "wc_seg.h"

namespace wc {
namespace {

// Two aligned chunks holding frame bytes from `at` on, each loaded only if it
// overlaps the frame (else the zero chunk): never a page the frame does not
// touch.
struct Win2 {
    u32x4 x, y;
};

__device__ __forceinline__ Win2 win2_load(uint64_t at, uint64_t fend, bool on, uint64_t zero)
{
    const uint64_t c = at & ~15ull;
    Win2 w;
    w.x = load_chunk<false>(on && c < fend ? c : zero);
    w.y = load_chunk<false>(on && c + 16u < fend ? c + 16u : zero);
    return w;
}

constexpr int kHdrChunks = 5; // an IPv4 header (<= 60 B) at any phase

// The header view shared by both parses: EtherType, version, IHL, lengths.
struct RxHdr {
    bool v4, v6, version_ok, hdr_in, frag, udp_in;
    uint32_t hl, room, proto, ip_plen;
};

__device__ __forceinline__ RxHdr rx_hdr(uint32_t f0, uint32_t f1, uint32_t f2, uint32_t flen)
{
    RxHdr x;
    const uint32_t etype = ((f0 & 0xFFu) << 8) | ((f0 >> 8) & 0xFFu); // eth.h:44-53
    const uint32_t b0 = (f0 >> 16) & 0xFFu;                              // vhl / vfc
    x.v4 = etype == 0x0800u;
    x.v6 = etype == 0x86DDu;
    x.room = flen >= 14u ? flen - 14u : 0u; // IP bytes inside the frame
    x.hl = x.v4 ? (b0 & 15u) * 4u : 40u;    // ip4.h:88-92, udp.c:113
    x.version_ok = (b0 >> 4) == (x.v4 ? 4u : 6u);
    // Header fields (ip4.h:55-66, ip6.h:45-57): valid once the header is in.
    x.hdr_in = (x.v4 || x.v6) && x.room >= 1u && x.version_ok &&
               x.room >= (x.v4 ? max(x.hl, 20u) : 40u);
    x.proto = x.v4 ? f2 >> 24 : f2 & 0xFFu; // p @9 / next_hdr @6
    // IP4_OFFMASK 0xff1f on the native word @6: the fragment offset (ip4.h:49)
    x.frag = x.v4 && (((f2 & 0x1Fu) | (f2 & 0xFF00u)) != 0u);
    x.ip_plen = x.v4 ? ((((f1 & 0xFFu) << 8) | ((f1 >> 8) & 0xFFu)) - x.hl) & 0xFFFFu // udp.c:104
                     : (((f1 >> 16) & 0xFFu) << 8) | (f1 >> 24);                     // udp.c:114
    x.udp_in = x.hdr_in && x.proto == 17u && x.ip_plen >= 8u && x.room >= x.hl + 8u;
    return x;
}

// The frame's first five aligned chunks (frame bytes [0, 65) at least, each
// chunk loaded only if it overlaps the frame): they hold the Ethernet header,
// an IPv4 header of up to 40 bytes or the IPv6 header, and the UDP length /
// checksum fields after either.
__device__ __forceinline__ void rx_load(uint64_t fa, uint32_t flen, bool valid, uint64_t zero,
                                        u32x4 (&c)[5])
{
    const uint64_t fend = fa + flen;
    const uint64_t cf = fa & ~15ull;
#pragma unroll
    for (int k = 0; k < 5; ++k)
        c[k] = load_chunk<false>(valid && cf + 16ull * k < fend ? cf + 16ull * k : zero);
}

} // namespace
} // namespace wc
