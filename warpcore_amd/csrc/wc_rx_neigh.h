// wc_rx_neigh.h -- what the RX neighbour kernels (wc_k_rxneigh.hip) and a host
// test share about one frame, each stated once: the
// decision chain of wc_rx_neigh_plan over an ARP frame or an ICMPv6 neighbour
// solicitation / advertisement, the (address, MAC) record neighbor_update
// receives, the 42 bytes of an ARP is-at and the 86 bytes of a neighbour
// advertisement as frame-relative dwords.  Plain C++ (no device builtin), so a
// host program compiles the same lines.  The engine table, eq16 and frame_dword
// are wc_rx_reply.h's; the 14-byte shift and the stores of the reply bytes at
// any 4-byte phase are wc_tx_build.h's (txb::shift14, store_words<N, N>).
//
// Reference decisions and stores restated (read, not copied; paths in the
// reference tree):
//   eth_rx     lib/src/eth.c:80-83       EtherType 08 06
//   arp_rx     lib/src/arp.c:157-198     formats, op, is_my_ip4(tpa, false), update
//   arp_is_at  lib/src/arp.c:65-100      the is-at frame
//   icmp6_rx   lib/src/icmp6.c:270-322   NADV / NSOL: target, option, update
//   icmp6_tx   lib/src/icmp6.c:168-193, 221-228   the advertisement
//   payload_cksum  lib/src/in_cksum.c:146-161
#pragma once

#include <stdint.h>

#include "wc_rx_reply.h"

namespace wc {
namespace rn {

// enum wc_rx_neigh_action (wc_cksum.h)
constexpr uint32_t kNone = 0, kMalformed = 4, kUpdate4 = 8, kArpIsAt = 9, kNadv = 10, kUpdate6 = 11;
constexpr uint32_t kMaskReply = 0x600u, kMaskUpdate = 0xF00u; // WC_RN_MASK_*
// Not an action code: the chain stops at a solicitation's target (chain_head).
constexpr uint32_t kTarget = 0x100u;
constexpr uint32_t kArpLen = 42u, kNadvLen = 86u, kTargetEnd = 78u;

WC_HD bool is_reply(uint32_t a)
{
    return a == kArpIsAt || a == kNadv;
}

WC_HD bool is_update(uint32_t a)
{
    return a >= kUpdate4 && a <= kUpdate6;
}

// What the chain reads of one frame in front of a solicitation's target: the
// reply plan's action byte, the frame length, frame bytes 12..15 / 16..19 /
// 20..23 / 38..41 as little-endian dwords and byte 54.  A field is looked at
// only behind the length check that places it inside the frame.
struct Look {
    uint32_t action, flen;
    uint32_t f3, f4, f5, tpa, b54;
};

// Steps 1 to 4 of the chain (wc_cksum.h, "RX neighbours"): the code, or kTarget
// for a solicitation whose target bytes 62..77 (inside the frame) decide.  A
// frame without an EtherType (flen < 14) has "any other EtherType".
WC_HD uint32_t chain_head(const uint32_t *e, const Look &f)
{
    if (f.action != rr::kHost || f.flen < 14u)
        return kNone;
    const uint32_t etype = f.f3 & 0xFFFFu; // as stored: 08 06 -> 0x0608
    if (etype == 0x0608u) {
        // w->have_ip4, and is_my_ip4(tpa, false) (ip4.c:200-214): addr alone
        bool have4 = false, mine = false;
        const uint32_t na = rr::eng_naddr(e);
        for (uint32_t k = 0; k < na; ++k) {
            const uint32_t *a = rr::eng_entry(e, k);
            if ((a[0] & 0xFFu) == 4u) {
                have4 = true;
                mine = mine || f.tpa == a[1];
            }
        }
        if (!have4)
            return kNone; // eth.c:80
        if (f.flen < kArpLen)
            return kMalformed;
        if ((f.f3 >> 16) != 0x0100u || ((f.f4 >> 16) & 0xFFu) != 6u) // hrd, hln (arp.c:161)
            return kNone;
        if ((f.f4 & 0xFFFFu) != 0x0008u || (f.f4 >> 24) != 4u) // pro, pln (arp.c:167)
            return kNone;
        const uint32_t op = f.f5 & 0xFFFFu;
        if (op == 0x0100u) // arp.c:179-183, 196
            return mine ? kArpIsAt : kUpdate4;
        return op == 0x0200u ? kUpdate4 : kNone;
    }
    if (etype != 0xDD86u)
        return kNone;
    if (f.flen < 55u || (f.f5 & 0xFFu) != 58u || (f.b54 != 135u && f.b54 != 136u))
        return kNone; // a stale action byte
    if (f.flen < kTargetEnd)
        return kMalformed;
    return f.b54 == 136u ? kUpdate6 : kTarget;
}

// Behind kTarget: is_my_ip6(target, false) over the af-6 entries (the reply
// plan's deliberate difference); icmp6.c:312-321: no update without a match.
WC_HD uint32_t chain_tail(const uint32_t *e, const uint32_t (&tgt)[4])
{
    bool mine = false;
    const uint32_t na = rr::eng_naddr(e);
    for (uint32_t k = 0; k < na; ++k) {
        const uint32_t *a = rr::eng_entry(e, k);
        mine = mine || ((a[0] & 0xFFu) == 6u && rr::eq16(tgt, a + 1));
    }
    return mine ? kNadv : kNone;
}

// struct wc_neigh_update as dwords: u[0] = af | action << 8 | mac[0..1] << 16,
// u[1] = mac[2..5], u[2..5] = addr.  All zero where the code is no update code
// or the frame is shorter than the bytes the code reads (42 / 78).
// Mem: ld32 (rr::frame_dword: aligned dwords that overlap the frame).
template <class Mem>
WC_HD void record_of(const Mem &m, uint64_t fa, uint32_t flen, uint32_t code, uint32_t (&u)[6])
{
    const uint64_t fend = fa + flen;
    u[0] = u[1] = u[2] = u[3] = u[4] = u[5] = 0u;
    uint32_t m0, m1; // the MAC's bytes 0..3 and 4..5
    if (code == kUpdate4 || code == kArpIsAt) {
        if (flen < kArpLen)
            return;
        m0 = rr::frame_dword(m, fa, fend, 22u); // sha, spa (arp.c:196-197)
        m1 = rr::frame_dword(m, fa, fend, 26u);
        u[2] = rr::frame_dword(m, fa, fend, 28u);
        u[0] = 4u;
    } else if (code == kUpdate6 || code == kNadv) {
        if (flen < kTargetEnd)
            return;
        // icmp6.c:272-282, 295-304: the option counts if data_len >= 24 and its
        // type and length bytes are 01 01 (bytes 78..85 then lie inside the frame)
        const uint32_t plen = txb::bswap16(rr::frame_dword(m, fa, fend, 18u) & 0xFFFFu);
        const uint32_t room = flen - 62u, dl = plen < room ? plen : room;
        bool opt = false;
        uint32_t o0 = 0u, o1 = 0u;
        if (dl >= 24u) {
            o0 = rr::frame_dword(m, fa, fend, 78u);
            o1 = rr::frame_dword(m, fa, fend, 82u);
            opt = (o0 & 0xFFFFu) == 0x0101u;
        }
        if (opt) {
            m0 = (o0 >> 16) | (o1 << 16);
            m1 = o1 >> 16;
        } else {
            m0 = rr::frame_dword(m, fa, fend, 6u);
            m1 = rr::frame_dword(m, fa, fend, 10u);
        }
        const uint32_t at = code == kNadv ? 22u : 62u; // ip->src (icmp6.c:316-318) / the target
        u[2] = rr::frame_dword(m, fa, fend, at);
        u[3] = rr::frame_dword(m, fa, fend, at + 4u);
        u[4] = rr::frame_dword(m, fa, fend, at + 8u);
        u[5] = rr::frame_dword(m, fa, fend, at + 12u);
        u[0] = 6u;
    } else {
        return;
    }
    u[0] |= (code << 8) | (m0 << 16);
    u[1] = (m0 >> 16) | (m1 << 16);
}

// The reply of `code` to the request at fa, written at da: its length, or 0
// with nothing written where the code is no reply code, the frame is shorter
// than the bytes the reply reads (42 / 78) or slot_bytes is below 42 / 86.
// Mem: ld32 / st8 / st16 / st32.
template <class Mem>
WC_HD uint32_t build(const Mem &m, uint64_t fa, uint32_t flen, uint32_t code, const uint32_t *e,
                     uint64_t da, uint32_t slot_bytes)
{
    const uint64_t fend = fa + flen;
    const uint32_t mac0 = e[0], mac1 = e[1] & 0xFFFFu;
    const uint32_t macw = (mac0 >> 16) | (mac1 << 16); // mac[2..5]
    if (code == kArpIsAt) {
        if (flen < kArpLen || slot_bytes < kArpLen)
            return 0u;
        // arp.c:78-96: dst = tha = the request's sha (not its Ethernet source),
        // spa = its tpa, tpa = its spa
        const uint32_t s0 = rr::frame_dword(m, fa, fend, 22u);
        const uint32_t s1 = rr::frame_dword(m, fa, fend, 26u) & 0xFFFFu;
        const uint32_t spa = rr::frame_dword(m, fa, fend, 28u);
        const uint32_t tpa = rr::frame_dword(m, fa, fend, 38u);
        uint32_t h[11];
        h[0] = s0;
        h[1] = s1 | (mac0 << 16);
        h[2] = macw;
        h[3] = 0x0608u | (0x0100u << 16); // 08 06, hrd 00 01
        h[4] = 0x04060008u;               // pro 08 00, hln 6, pln 4
        h[5] = 0x0200u | (mac0 << 16);    // op 00 02, sha
        h[6] = macw;
        h[7] = tpa;
        h[8] = s0;
        h[9] = s1 | (spa << 16);
        h[10] = spa >> 16;
        txb::store_words<11, 11>(m, da, true, h);
        return kArpLen;
    }
    if (code != kNadv || flen < kTargetEnd || slot_bytes < kNadvLen)
        return 0u;
    // icmp6.c:168-193, 221-228.  The source-link-address test there reads the
    // ICMPv6 type and code bytes (a type of 135 is never 1), so the Ethernet
    // destination is always the request's source MAC.
    const uint32_t d0 = rr::frame_dword(m, fa, fend, 6u);
    const uint32_t d1 = rr::frame_dword(m, fa, fend, 10u) & 0xFFFFu;
    const uint32_t *s = rr::eng_entry(e, 0u) + 1; // entry 0's address (ip6.c:155)
    uint32_t ip[18];
    ip[0] = 0x60u; // the whole word, as the existing replies write it
    ip[1] = 0x2000u | (58u << 16) | (0xFFu << 24); // len 00 20, next header, hop limit
    ip[10] = 0x0088u; // type 136, code 0, checksum 0
    ip[11] = 0x60u;   // Solicited + Override (icmp6.c:169-170)
    ip[16] = 0x0102u | (mac0 << 16); // option 02 01, then mac
    ip[17] = macw;
    // payload_cksum(ip, 72) as in_cksum.c:146-161 forms it: next header << 24,
    // the address words, the length word, then the 32 ICMPv6 bytes' words.
    // 58 << 24 plus 33 words stays below 2^32.
    uint32_t S = (58u << 24) + 0x2000u + txb::words(ip[10]) + txb::words(ip[11]) +
                 txb::words(ip[16]) + txb::words(ip[17]);
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 0; k < 4; ++k) {
        ip[2 + k] = s[k];
        ip[6 + k] = rr::frame_dword(m, fa, fend, 22u + 4u * k);  // the request's source
        ip[12 + k] = rr::frame_dword(m, fa, fend, 62u + 4u * k); // the target
        S += txb::words(ip[2 + k]) + txb::words(ip[6 + k]) + txb::words(ip[12 + k]);
    }
    ip[10] |= txb::fold_not16(S) << 16; // icmp6.c:72-73, stored raw
    uint32_t h[22];
    h[0] = d0;
    h[1] = d1 | (mac0 << 16);
    h[2] = macw;
    txb::shift14(0xDD86u, ip, h);
    txb::store_words<22, 22>(m, da, true, h);
    return kNadvLen;
}

} // namespace rn
} // namespace wc
