// wc_rx_reply.h -- what the RX reply kernels (wc_k_rxreply.hip) and a host
// test share about one frame, each stated once: the
// engine table as little-endian dwords, the address filters, the decision
// chain of wc_rx_reply_plan, the lengths and bounds of every reply (which the
// build derives again), the 42 or 62 header bytes of a reply as frame-relative
// dwords, and the gather-copy of a reply's data with its sum, one aligned
// destination chunk or dword at a time.  Plain C++ (no device builtin), so a
// host program compiles the same lines.  The byte swap, the folds, the 14-byte
// shift and the header stores are the TX build's (txb::bswap16, fold16,
// shift14, store_headers).
//
// Reference decisions and stores restated (read, not copied):
//   eth_rx     /root/reference/lib/src/eth.c:65-73      MAC filter
//   ip4_rx     /root/reference/lib/src/ip4.c:103-137    is_my_ip4, protocol unreachable
//   is_my_ip4  /root/reference/lib/src/ip4.c:200-214
//   ip6_rx     /root/reference/lib/src/ip6.c:98-111     is_my_ip6
//   is_my_ip6  /root/reference/lib/src/ip6.c:173-187
//   udp_rx     /root/reference/lib/src/udp.c:144-155    port unreachable
//   icmp4_rx / icmp4_tx  /root/reference/lib/src/icmp4.c:56-129, 144-196
//   icmp6_rx / icmp6_tx  /root/reference/lib/src/icmp6.c:55-78, 140-231, 250-267
//   mk_ip4_hdr(v, 0) / mk_ip6_hdr(v, 0)  ip4.c:153-189, ip6.c:127-161
#pragma once

#include <stdint.h>

#include "wc_tx_build.h"

namespace wc {
namespace rr {

// enum wc_rx_reply_action (wc_cksum.h)
constexpr uint32_t kNone = 0, kHost = 1, kFiltered = 2, kIcmpBadCksum = 3, kMalformed = 4,
                   kNoRoom = 5, kEcho4 = 8, kEcho6 = 9, kUnreachPort4 = 10, kUnreachPort6 = 11,
                   kUnreachProto4 = 12;
constexpr uint32_t kMaskReply = 0x1F00u; // WC_RR_MASK_REPLY
// Not action codes: the chain stops at an ICMP / ICMPv6 sum (chain_head).
constexpr uint32_t kSum4 = 0x100, kSum6 = 0x101;
// enum wc_rx_verdict: the four codes that are no drop; WC_RX_SOCK_UNBOUND
constexpr uint32_t kRxOk = 0, kRxOkNoCksum = 1, kRxNotUdp = 7, kRxNotIp = 8;
constexpr uint32_t kSockUnbound = 0xFFu;

// struct wc_rx_engine as dwords: e[0] = mac[0..3], e[1] = mac[4..5] | mtu << 16,
// e[2] = naddr, then WC_RX_MAX_IFADDR entries of 13: a[0] = af | pad << 8,
// a[1..4] = addr, a[5..8] = bcast, a[9..12] = snma.
constexpr uint32_t kMaxIfaddr = 16, kIfaddrWords = 13, kEngineWords = 3 + kMaxIfaddr * kIfaddrWords;

using txb::fold16; // rr::fold16: the fold of a reply's data sum (headers' `data`)

WC_HD bool is_reply(uint32_t a)
{
    return a < 32u && ((kMaskReply >> a) & 1u);
}

WC_HD bool reply_v4(uint32_t a)
{
    return a == kEcho4 || a == kUnreachPort4 || a == kUnreachProto4;
}

WC_HD uint32_t eng_mtu(const uint32_t *e)
{
    return e[1] >> 16;
}

// (a table wc_rx_engine_check refuses still reads inside the struct)
WC_HD uint32_t eng_naddr(const uint32_t *e)
{
    return e[2] < kMaxIfaddr ? e[2] : kMaxIfaddr;
}

// Address entry k: a[0] = af, a[1..4] = addr, a[5..8] = bcast, a[9..12] = snma.
WC_HD const uint32_t *eng_entry(const uint32_t *e, uint32_t k)
{
    return e + 3u + kIfaddrWords * k;
}

// eth.c:65-67 on frame bytes 0..3 (d0) and 4..7 (d1): ours, broadcast, or
// 33 33 in bytes 0..1.
WC_HD bool mac_ok(const uint32_t *e, uint32_t d0, uint32_t d1)
{
    const uint32_t lo = d1 & 0xFFFFu;
    return (d0 == e[0] && lo == (e[1] & 0xFFFFu)) || (d0 == 0xFFFFFFFFu && lo == 0xFFFFu) ||
           (d0 & 0xFFFFu) == 0x3333u;
}

WC_HD bool eq16(const uint32_t (&x)[4], const uint32_t *a)
{
    return x[0] == a[0] && x[1] == a[1] && x[2] == a[2] && x[3] == a[3];
}

// is_my_ip4 / is_my_ip6 over the table.  dst: with the broadcast match
// (ip4.c:103, ip6.c:98); src: without (udp.c:150-153).  IPv4 addresses are
// d[0] / s[0].  Entries of the other family never match: for IPv6 that is the
// deliberate difference from the reference's loop (wc_cksum.h).
struct Match {
    bool dst, src;
};

WC_HD Match addr_match(const uint32_t *e, bool v4, const uint32_t (&d)[4], const uint32_t (&s)[4])
{
    bool d4 = false, s4 = false, d6 = false, s6 = false;
    const uint32_t na = eng_naddr(e);
    for (uint32_t k = 0; k < na; ++k) {
        const uint32_t *a = eng_entry(e, k);
        const uint32_t af = a[0] & 0xFFu;
        if (af == 4u) {
            d4 = d4 || d[0] == a[1] || d[0] == a[5] || d[0] == 0xFFFFFFFFu;
            s4 = s4 || s[0] == a[1];
        } else if (af == 6u) {
            d6 = d6 || eq16(d, a + 1) || eq16(d, a + 9) || eq16(d, a + 5);
            s6 = s6 || eq16(s, a + 1);
        }
    }
    return Match{v4 ? d4 : d6, v4 ? s4 : s6};
}

// The first af-4 address (ifaddr[addr4_pos], ip4.c:180); 0 without one.
WC_HD uint32_t eng_src4(const uint32_t *e)
{
    const uint32_t na = eng_naddr(e);
    uint32_t src = 0u;
    bool found = false;
    for (uint32_t k = 0; k < na; ++k) {
        const uint32_t *a = eng_entry(e, k);
        if (!found && (a[0] & 0xFFu) == 4u) {
            src = a[1];
            found = true;
        }
    }
    return src;
}

// One reply's lengths: the frame length `len`, and the request bytes [s0, s0 +
// dlen) that follow its headers.  action: the reply action, or kMalformed /
// kNoRoom with every length 0.
struct Reply {
    uint32_t action, len, s0, dlen;
};

// The lengths and bounds of a reply action on a frame of flen bytes: hl = 4 *
// IHL as the byte gives it, ip_len = ip->len (IPv4 actions) or ip6->len.  The
// plan calls it where the chain arrives at a reply, the build on the action
// byte it is handed, so a stale byte cannot name a byte outside the frame or
// the slot.  32-bit arithmetic; the one wrap the reference has (icmp4.c:91,
// icmp6.c:202 in a uint16) is the t < hl + 8 / t < 8 check.  The first check
// of each branch -- the fixed header bytes a reply reads lie inside the frame
// -- holds for every frame the RX verdict lets through to here.
WC_HD Reply reply_of(uint32_t action, uint32_t hl, uint32_t ip_len, uint32_t flen, uint32_t mtu,
                     uint32_t slot_bytes)
{
    Reply r{action, 0u, 0u, 0u};
    bool bad;
    if (action == kEcho4) {
        const uint32_t t = ip_len < mtu ? ip_len : mtu; // icmp4.c:80
        bad = flen < 34u || t < hl + 8u || 14u + t > flen;
        r.s0 = 14u + hl + 8u;
        r.dlen = t - hl - 8u;
        r.len = 42u + r.dlen;
    } else if (action == kUnreachPort4 || action == kUnreachProto4) {
        bad = flen < 34u || flen < 14u + hl + 8u; // icmp4.c:99, 107
        r.s0 = 14u;
        r.dlen = hl + 8u;
        r.len = 50u + hl;
    } else if (action == kEcho6) {
        const uint32_t room = mtu - 40u; // (mtu >= 68: wc_rx_engine_check)
        const uint32_t t = ip_len < room ? ip_len : room; // icmp6.c:164
        bad = flen < 54u || t < 8u || 54u + t > flen;
        r.s0 = 62u;
        r.dlen = t - 8u;
        r.len = 62u + r.dlen;
    } else { // kUnreachPort6: 48 bytes from ip6_data(buf) (icmp6.c:163, 210)
        bad = flen < 102u;
        r.s0 = 54u;
        r.dlen = 48u;
        r.len = 110u;
    }
    if (bad)
        r = Reply{kMalformed, 0u, 0u, 0u};
    else if (r.len > slot_bytes)
        r = Reply{kNoRoom, 0u, 0u, 0u};
    return r;
}

// What the chain reads of one frame.
struct Frame {
    uint32_t verdict, flen;
    bool unbound;                // d_sock given and d_sock[i] == WC_RX_SOCK_UNBOUND
    bool mac_ok, dst_ok, src_ok; // the filters above
    bool v4;                     // EtherType 08 00 (else 86 dd, where it matters)
    uint32_t hl, proto, ip_len;  // 4 * IHL or 40; protocol / next header; ip->len / ip6->len
};

// Steps 1 to 6 and 8 of the chain (wc_cksum.h, "RX replies"): the action, or
// kSum4 / kSum6 where it depends on a sum -- sum_len = the bytes of
// ip_cksum(ip + hl, sum_len) or payload_cksum(ip, sum_len) to take.
WC_HD Reply chain_head(const Frame &f, uint32_t mtu, uint32_t slot_bytes, uint32_t &sum_len)
{
    sum_len = 0u;
    const uint32_t v = f.verdict;
    if (v != kRxOk && v != kRxOkNoCksum && v != kRxNotUdp && v != kRxNotIp)
        return Reply{kNone, 0u, 0u, 0u};
    if (!f.mac_ok)
        return Reply{kFiltered, 0u, 0u, 0u};
    if (v == kRxNotIp)
        return Reply{kHost, 0u, 0u, 0u};
    if (!f.dst_ok)
        return Reply{kFiltered, 0u, 0u, 0u};
    // (every verdict left has placed the IP header inside the frame; a verdict
    // byte that lies must not move a sum past it)
    if (f.flen < 14u + (f.v4 ? (f.hl > 20u ? f.hl : 20u) : 40u))
        return Reply{kMalformed, 0u, 0u, 0u};
    if (v != kRxNotUdp) {
        // udp.c:150-153 asks is_my_ip4 / is_my_ip6 about the frame's SOURCE
        // address: the reference's behaviour, not a typo of ours.
        if (!f.unbound || !f.src_ok)
            return Reply{kNone, 0u, 0u, 0u};
        return reply_of(f.v4 ? kUnreachPort4 : kUnreachPort6, f.hl, f.ip_len, f.flen, mtu,
                        slot_bytes);
    }
    if (f.v4) {
        if (f.proto != 1u)
            return reply_of(kUnreachProto4, f.hl, f.ip_len, f.flen, mtu, slot_bytes);
        const uint32_t a = (f.ip_len - f.hl) & 0xFFFFu, b = f.flen - 14u - f.hl; // icmp4.c:153-154
        sum_len = a < b ? a : b;
        return Reply{kSum4, 0u, 0u, 0u};
    }
    if (f.proto != 58u)
        return Reply{kNone, 0u, 0u, 0u};
    const uint32_t b = f.flen - 54u; // icmp6.c:259-261
    sum_len = (f.ip_len < b ? f.ip_len : b) + 40u;
    return Reply{kSum6, 0u, 0u, 0u};
}

// Steps 7 and 9 behind the sum: ck = its value (ip_cksum of no byte is
// 0xFFFF), type = the ICMP type byte at frame byte 14 + hl / 54 (read only
// where it lies inside the frame).
WC_HD Reply chain_tail(uint32_t stage, const Frame &f, uint32_t ck, uint32_t type, uint32_t mtu,
                       uint32_t slot_bytes)
{
    if (ck != 0u)
        return Reply{kIcmpBadCksum, 0u, 0u, 0u};
    if (stage == kSum4) {
        if (type != 8u)
            return Reply{kNone, 0u, 0u, 0u};
        return reply_of(kEcho4, f.hl, f.ip_len, f.flen, mtu, slot_bytes);
    }
    if (f.flen < 55u)
        return Reply{kMalformed, 0u, 0u, 0u};
    if (type == 135u || type == 136u)
        return Reply{kHost, 0u, 0u, 0u};
    if (type == 128u)
        return reply_of(kEcho6, f.hl, f.ip_len, f.flen, mtu, slot_bytes);
    return Reply{kNone, 0u, 0u, 0u};
}

// Frame bytes [at, at + 4) as a little-endian dword, from the one or two
// aligned dwords that hold them -- each loaded only if it overlaps the frame
// [fa, fend).  Mem: ld32(address).
template <class Mem>
WC_HD uint32_t frame_dword(const Mem &m, uint64_t fa, uint64_t fend, uint32_t at)
{
    const uint64_t s = fa + at, a = s & ~3ull;
    const uint32_t sh = 8u * (uint32_t)(s & 3u);
    const uint32_t lo = a + 4u > fa && a < fend ? m.ld32(a) : 0u;
    if (sh == 0u)
        return lo;
    const uint32_t hi = a + 4u < fend ? m.ld32(a + 4u) : 0u;
    return (lo >> sh) | (hi << (32u - sh));
}

// What a reply takes from the request beside its data bytes.
struct Req {
    uint32_t smac0, smac1; // frame bytes 6..9 and 10..11: the reply's Ethernet dst
    uint32_t src[4];       // the IP source (IPv4: src[0]): the reply's IP dst
    uint32_t rest;         // an echo's ICMP bytes 4..7 as stored; 0 for an unreachable
};

// The bytes named above lie inside the frame for every Reply reply_of passes.
template <class Mem>
WC_HD Req request_of(const Mem &m, uint64_t fa, uint64_t fend, uint32_t action, uint32_t hl)
{
    Req q;
    q.smac0 = frame_dword(m, fa, fend, 6u);
    q.smac1 = frame_dword(m, fa, fend, 10u) & 0xFFFFu;
    const bool v4 = reply_v4(action);
    q.src[0] = frame_dword(m, fa, fend, v4 ? 26u : 22u);
    q.src[1] = q.src[2] = q.src[3] = 0u;
    if (!v4) {
        q.src[1] = frame_dword(m, fa, fend, 26u);
        q.src[2] = frame_dword(m, fa, fend, 30u);
        q.src[3] = frame_dword(m, fa, fend, 34u);
    }
    q.rest = 0u;
    if (action == kEcho4)
        q.rest = frame_dword(m, fa, fend, 14u + hl + 4u);
    else if (action == kEcho6)
        q.rest = frame_dword(m, fa, fend, 58u);
    return q;
}

// The 42 (IPv4) or 62 (IPv6) header bytes of a reply as little-endian dwords
// from its first byte (the layout of txb::Hdr::h, stored by
// txb::store_headers).  data = the sum of the data's little-endian words
// from its first byte on -- copy_dword's and copy_chunk's shares summed (below
// 2^32 for any dlen <= 65535 across a wave: 32768 words) and folded to 16 bits
// (rr::fold16 = txb::fold16).
//
// No sum wraps.  ip_cksum of the IPv4 header: ten words.  The ICMP sum
// (icmp4.c:111): four header words and one folded data word, below 2^19.  The
// ICMPv6 sum (payload_cksum, in_cksum.c:155-164): 58 << 24 plus 16 address
// words, the length word, four header words and the folded data word, below
// 2^30; the reference's own accumulator adds the data's <= 32764 words
// unfolded and stays below 2^32 too (58 << 24 + 32800 * 0xFFFF < 0xBB000000),
// so both are positive numbers with the same residue mod 0xFFFF and fold alike.
WC_HD void headers(const Reply &r, const Req &q, const uint32_t *e, uint32_t ip_id, uint32_t data,
                   uint32_t (&h)[16])
{
    using txb::bswap16;
    using txb::fold_not16;
    using txb::words;
    const bool v4 = reply_v4(r.action);
    // type, code (icmp4.h / icmp6.h): echo reply 0 / 129, unreachable 3 / 1
    // with code port 3 / 4 or protocol 2
    const uint32_t tc = r.action == kEcho4          ? 0x0000u
                        : r.action == kEcho6        ? 0x0081u
                        : r.action == kUnreachPort4 ? 0x0303u
                        : r.action == kUnreachPort6 ? 0x0401u
                                                    : 0x0203u;
    uint32_t ip[12];
    if (v4) {
        const uint32_t src = eng_src4(e);
        const uint32_t a0 = 0x45u | (bswap16(r.len - 14u) << 16); // vhl, tos 0 (v->flags = 0), len
        const uint32_t a1 = (ip_id & 0xFFFFu) | (0x0040u << 16);  // id as stored, DF
        const uint32_t a2 = 0xFFu | (1u << 8);                    // ttl, IP_P_ICMP
        const uint32_t ick = fold_not16(words(a0) + words(a1) + words(a2) + words(src) +
                                        words(q.src[0])); // ip4.c:185-186
        const uint32_t ck = fold_not16(words(tc) + words(q.rest) + data); // icmp4.c:110-111
        ip[0] = a0, ip[1] = a1, ip[2] = a2 | (ick << 16), ip[3] = src, ip[4] = q.src[0];
        ip[5] = tc | (ck << 16), ip[6] = q.rest;
        ip[7] = ip[8] = ip[9] = ip[10] = ip[11] = 0u;
    } else {
        const uint32_t *s = eng_entry(e, 0u) + 1;     // entry 0's address (ip6.c:155)
        const uint32_t plen = bswap16(r.len - 54u);   // ip6->len as stored
        uint32_t S = (58u << 24) + plen + words(tc) + words(q.rest) + data;
#if defined(__clang__)
#pragma unroll
#endif
        for (int k = 0; k < 4; ++k)
            S += words(s[k]) + words(q.src[k]);
        const uint32_t ck = fold_not16(S); // icmp6.c:72-73
        ip[0] = 0x60u; // the whole word: the TX build's deliberate difference (wc_cksum.h)
        ip[1] = plen | (58u << 16) | (0xFFu << 24);
#if defined(__clang__)
#pragma unroll
#endif
        for (int k = 0; k < 4; ++k)
            ip[2 + k] = s[k], ip[6 + k] = q.src[k];
        ip[10] = tc | (ck << 16), ip[11] = q.rest;
    }
    // ... 14 bytes into the frame: behind dst = the request's src, src = mac, type
    h[0] = q.smac0;
    h[1] = q.smac1 | (e[0] << 16);
    h[2] = (e[0] >> 16) | (e[1] << 16);
    txb::shift14(v4 ? 0x0008u : 0xDD86u, ip, h);
}

// The aligned dwords a reply's data [dd, dd + dlen) touches.
WC_HD uint32_t copy_dwords(uint64_t dd, uint32_t dlen)
{
    return dlen ? ((uint32_t)(dd & 3u) + dlen + 3u) >> 2 : 0u;
}

// One of them: destination dword i (< copy_dwords) lies at (dd & ~3) + 4 i and
// takes data bytes [4 i - pd, + 4) with pd = dd & 3 -- source bytes from sa +
// 4 i - pd on, assembled from the two aligned source dwords that hold them
// (each loaded only if it overlaps [sa, sa + dlen)).  Whole dwords are stored
// whole, the data's two ends as byte / 2-byte stores at their natural
// alignment: no byte outside [dd, dd + dlen) is written.  Returns the dword's
// share of the sum of the data's little-endian words from its first byte on
// (csum_oc16 over the bytes as written: a byte at an odd data offset counts
// 256-fold); a lane's shares of a 65535-byte data stay below 2^31.
// Mem: ld32 / st8 / st16 / st32.
template <class Mem>
WC_HD uint32_t copy_dword(const Mem &m, uint64_t sa, uint64_t dd, uint32_t dlen, uint32_t i)
{
    const uint32_t pd = (uint32_t)(dd & 3u);
    const uint64_t s = sa + 4ull * i - pd, a = s & ~3ull, se = sa + dlen;
    const uint32_t sh = 8u * (uint32_t)(s & 3u);
    const uint32_t lo = a + 4u > sa && a < se ? m.ld32(a) : 0u;
    uint32_t v = lo;
    if (sh != 0u) {
        const uint32_t hi = a + 8u > sa && a + 4u < se ? m.ld32(a + 4u) : 0u;
        v = (lo >> sh) | (hi << (32u - sh));
    }
    const uint32_t b0 = i ? 0u : pd;        // the dword's bytes [b0, b1) are data
    const uint32_t rem = pd + dlen - 4u * i;
    const uint32_t b1 = rem < 4u ? rem : 4u;
    const uint32_t keep = (b1 >= 4u ? 0xFFFFFFFFu : (1u << (8u * b1)) - 1u) & ~((1u << (8u * b0)) - 1u);
    v &= keep;
    const uint64_t da = (dd & ~3ull) + 4ull * i;
    if (b0 == 0u && b1 == 4u) {
        m.st32(da, v);
    } else {
        if (b0 == 0u && b1 >= 2u) {
            m.st16(da, v & 0xFFFFu);
        } else {
            if (b0 == 0u)
                m.st8(da, v & 0xFFu);
            if (b0 <= 1u && b1 >= 2u)
                m.st8(da + 1u, (v >> 8) & 0xFFu);
        }
        if (b0 <= 2u && b1 == 4u) {
            m.st16(da + 2u, v >> 16);
        } else {
            if (b0 <= 2u && b1 >= 3u)
                m.st8(da + 2u, (v >> 16) & 0xFFu);
            if (b1 == 4u)
                m.st8(da + 3u, v >> 24);
        }
    }
    // byte b of the dword is data byte 4 i - pd + b: odd with pd + b
    const uint32_t w = (pd & 1u) ? ((v & 0x00FF00FFu) << 8) | ((v >> 8) & 0x00FF00FFu) : v;
    return txb::words(w);
}

// The same for the aligned 16-byte chunks that lie wholly inside the data:
// chunk c lies at (dd & ~15) + 16 c, and those with c0 <= c < c1 are copied
// whole (copy_chunk) -- in terms of copy_dword's index the dwords [i0, i1),
// which it then leaves out; with no whole chunk the range is empty.
struct Quad {
    uint32_t x, y, z, w;
};

struct Chunks {
    uint32_t c0, c1, i0, i1;
};

WC_HD Chunks copy_chunks(uint64_t dd, uint32_t dlen)
{
    const uint32_t p = (uint32_t)(dd & 15u), pq = p >> 2;
    Chunks k;
    k.c0 = p ? 1u : 0u;
    k.c1 = (p + dlen) >> 4;
    if (k.c1 <= k.c0) {
        k.c0 = k.c1 = k.i0 = k.i1 = 0u;
    } else {
        k.i0 = 4u * k.c0 - pq;
        k.i1 = 4u * k.c1 - pq;
    }
    return k;
}

// Chunk c (c0 <= c < c1): sixteen data bytes from offset 16 c - (dd & 15) on,
// assembled from the two aligned 16-byte source chunks that hold them (the
// second loaded only if the source phase needs it; both overlap [sa, sa +
// dlen)) and stored whole.  The source phase is the same for every chunk of a
// reply.  Returns the chunk's share of the sum, as copy_dword.
// Mem: ld128 / st128 on Quad.
template <class Mem>
WC_HD uint32_t copy_chunk(const Mem &m, uint64_t sa, uint64_t dd, uint32_t c)
{
    const uint64_t s = sa + 16ull * c - (dd & 15u), a = s & ~15ull;
    const uint32_t sh = (uint32_t)(s & 15u), bs = 8u * (sh & 3u);
    const Quad X = m.ld128(a);
    Quad Y{0u, 0u, 0u, 0u};
    if (sh != 0u)
        Y = m.ld128(a + 16u);
    // the window's dwords q .. q + 4 of X:Y, q = sh >> 2, in two select levels
    const bool q1 = sh & 4u, q2 = sh & 8u;
    const uint32_t e0 = q1 ? X.y : X.x, e1 = q1 ? X.z : X.y, e2 = q1 ? X.w : X.z,
                   e3 = q1 ? Y.x : X.w, e4 = q1 ? Y.y : Y.x, e5 = q1 ? Y.z : Y.y,
                   e6 = q1 ? Y.w : Y.z;
    const uint32_t d0 = q2 ? e2 : e0, d1 = q2 ? e3 : e1, d2 = q2 ? e4 : e2, d3 = q2 ? e5 : e3,
                   d4 = q2 ? e6 : e4;
    Quad o{d0, d1, d2, d3};
    if (bs != 0u) {
        const uint32_t ls = 32u - bs;
        o = Quad{(d0 >> bs) | (d1 << ls), (d1 >> bs) | (d2 << ls), (d2 >> bs) | (d3 << ls),
                 (d3 >> bs) | (d4 << ls)};
    }
    m.st128((dd & ~15ull) + 16ull * c, o);
    if (dd & 1u) { // a byte at an odd data offset counts 256-fold
        o.x = ((o.x & 0x00FF00FFu) << 8) | ((o.x >> 8) & 0x00FF00FFu);
        o.y = ((o.y & 0x00FF00FFu) << 8) | ((o.y >> 8) & 0x00FF00FFu);
        o.z = ((o.z & 0x00FF00FFu) << 8) | ((o.z >> 8) & 0x00FF00FFu);
        o.w = ((o.w & 0x00FF00FFu) << 8) | ((o.w >> 8) & 0x00FF00FFu);
    }
    return txb::words(o.x) + txb::words(o.y) + txb::words(o.z) + txb::words(o.w);
}

} // namespace rr
} // namespace wc
