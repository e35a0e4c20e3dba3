// wc_rx_socktab.h -- the RX demultiplex socket table (wc_rx_socktab_*,
// wc_rx_demux): its layout, hash and probe, shared word for word by the host
// (wc_rt_rx.cpp: build, lookup) and the device (wc_k_rxdemux.hip: the LDS
// copy's probe), so the two cannot drift apart.
//
// What it answers is the reference's w_get_sock (backend_netmap.c:481-490):
// an exact compare of the whole tuple (warpcore.c:644-677).  The hash below
// is this project's own; it needs only to be the same on both sides.
//
// Blob: a 16-byte header {magic, slots, ns, 0} and `slots` 48-byte slots, an
// open-addressing table with linear probing.  A slot is 12 little-endian
// dwords: the socket's canonical key -- struct wc_rx_sock's own 40 bytes with
// every ignored byte 0 (pad; bytes 4..15 of an IPv4 address; rport and raddr
// of a bound-only socket) --, its index (kTabEmpty: a free slot) and a zero
// dword.  slots is a power of two >= 2 ns + 2, so a probe always meets a free
// slot.  No pointer inside: the blob may be copied anywhere.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define WC_TAB_HD __host__ __device__ inline
#else
#define WC_TAB_HD inline
#endif

namespace wc {
namespace tab {

constexpr uint32_t kTabMagic = 0x62745357u; // "WStb"
constexpr uint32_t kTabMaxSocks = 254;
constexpr uint32_t kTabHeaderWords = 4;
constexpr uint32_t kTabKeyWords = 10;
constexpr uint32_t kTabSlotWords = 12;
constexpr uint32_t kTabEmpty = 0xFFFFFFFFu;
constexpr uint32_t kTabUnbound = 0xFFu; // WC_RX_SOCK_UNBOUND

// Slots of a table of ns sockets: the power of two >= 2 ns + 2 (at least 4).
WC_TAB_HD constexpr uint32_t tab_slots(uint32_t ns)
{
    uint32_t s = 4;
    while (s < 2u * ns + 2u)
        s <<= 1;
    return s;
}

WC_TAB_HD constexpr uint32_t tab_words(uint32_t ns)
{
    return kTabHeaderWords + kTabSlotWords * tab_slots(ns);
}

// A tuple as the table keys it.  conn: 1 the connected four-tuple, 0 the
// bound-only pair (remote ignored).  l / r: the addresses' dwords as they lie
// in the packet (IPv4: word 0 only).
WC_TAB_HD void tab_key(uint32_t k[kTabKeyWords], uint32_t af, uint32_t conn, uint32_t lport,
                       uint32_t rport, const uint32_t l[4], const uint32_t r[4])
{
    const bool v4 = af == 4u;
    k[0] = af | (conn << 8) | (lport << 16);
    k[1] = conn ? rport : 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const bool live = j == 0 || !v4;
        k[2 + j] = live ? l[j] : 0u;
        k[6 + j] = live && conn ? r[j] : 0u;
    }
}

// The bound-only key of the same local pair as the connected key k.
WC_TAB_HD void tab_key_bound(uint32_t b[kTabKeyWords], const uint32_t k[kTabKeyWords])
{
    b[0] = k[0] & ~0xFF00u;
    b[1] = 0u;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        b[2 + j] = k[2 + j];
        b[6 + j] = 0u;
    }
}

WC_TAB_HD uint32_t tab_hash(const uint32_t k[kTabKeyWords])
{
    uint32_t h = 0x9E3779B9u;
#pragma unroll
    for (uint32_t j = 0; j < kTabKeyWords; ++j) {
        h = (h ^ k[j]) * 0x85EBCA6Bu;
        h ^= h >> 13;
    }
    h *= 0xC2B2AE35u;
    return h ^ (h >> 16);
}

// The index stored with key k among `slots` slots at `s`, or kTabEmpty.  At
// most `slots` steps, whatever the bytes hold.
template <class Words>
WC_TAB_HD uint32_t tab_find(Words s, uint32_t slots, const uint32_t k[kTabKeyWords])
{
    uint32_t at = tab_hash(k) & (slots - 1u);
    for (uint32_t step = 0; step < slots; ++step) {
        const uint32_t o = at * kTabSlotWords;
        const uint32_t idx = s[o + kTabKeyWords];
        if (idx == kTabEmpty)
            return kTabEmpty;
        bool same = true;
#pragma unroll
        for (uint32_t j = 0; j < kTabKeyWords; ++j)
            same = same && s[o + j] == k[j];
        if (same)
            return idx;
        at = (at + 1u) & (slots - 1u);
    }
    return kTabEmpty;
}

// udp_rx's two steps (udp.c:143-146): the connected tuple, then the bound one.
template <class Words>
WC_TAB_HD uint32_t tab_lookup(Words s, uint32_t slots, const uint32_t k[kTabKeyWords])
{
    uint32_t idx = tab_find(s, slots, k);
    if (idx == kTabEmpty) {
        uint32_t b[kTabKeyWords];
        tab_key_bound(b, k);
        idx = tab_find(s, slots, b);
    }
    return idx == kTabEmpty ? kTabUnbound : idx;
}

} // namespace tab
} // namespace wc
