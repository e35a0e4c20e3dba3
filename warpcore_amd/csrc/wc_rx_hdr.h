// wc_rx_hdr.h -- what the RX verdict kernel (wc_k_rx.hip) and the TX seal
// kernel (wc_k_tx.hip) share about one frame, each stated once (DESIGN.md
// sections 8 and 4.7):
//   * the per-frame header chunk loads that stay inside the frame (win2_load,
//     rx_load);
//   * the header view both decision chains read (RxHdr: EtherType, version,
//     IHL, lengths, fragment offset, protocol / next header);
//   * the frame header parse (FrameHdr): that view, the UDP length / checksum
//     word and ip_cksum(ip, hl) of the header as loaded -- frame_hdr over
//     rx_load's five chunks (IPv4 headers of 20..40 bytes), frame_hdr_slow in
//     two load rounds of its own (any IHL);
//   * frame bytes 0..55 as dwords out of the same five chunks (rx_words56: the
//     RX reply and RX neighbour plans, wc_k_rxreply.hip / wc_k_rxneigh.hip);
//   * the gathered stream of a tile's frames that need the UDP sum (FrameLds,
//     frame_payload_cksum).
//   * the RX decision chain and the delivery record (rx_decide, rx_record,
//     rx_parse_rec, rx_parse_slow_rec), at the end of this file: the RX verdict
//     kernels' and the RX drain kernel's (wc_k_rxdrain.hip).
// The TX seal's chain (tx_decide) restates other reference functions and stays
// with its kernel.
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

// Frame bytes 0..55 as fourteen dwords (A: bytes 0..19, B: 20..39, C: 40..55):
// three 20-byte windows rotated out of rx_load's five chunks (frame_hdr's way).
// What the RX reply and RX neighbour plans read of a frame.
__device__ __forceinline__ void rx_words56(const u32x4 (&c)[5], uint64_t fa, uint32_t (&A)[5],
                                           uint32_t (&B)[5], uint32_t (&C)[4])
{
    const uint32_t sf = (uint32_t)(fa & 15u);
    const u32x4 z4 = {0u, 0u, 0u, 0u};
    win_rot(c[0], c[1], c[2], sf, A);
    const uint32_t o1 = sf + 20u, o2 = sf + 40u;
    const bool j1 = o1 >= 32u, j2 = o2 >= 48u;
    win_rot(j1 ? c[2] : c[1], j1 ? c[3] : c[2], j1 ? c[4] : c[3], o1 & 15u, B);
    win_rot(j2 ? c[3] : c[2], j2 ? c[4] : c[3], j2 ? z4 : c[4], o2 & 15u, C);
}

// What either kernel's decision chain takes from the frame's headers.
struct FrameHdr {
    RxHdr x;
    uint32_t g0;   // UDP length | checksum << 16 (udp.h:41-46), a native word
    uint32_t ipck; // ip_cksum(ip, hl) of the header as loaded
    uint32_t f_ip; // ip->cksum as loaded, a native word (the TX seal only)
    // What a delivery record takes beside these (the RX DELIVER kernels only;
    // 0 from a parse without EXTRA, so every other kernel compiles as before):
    uint32_t pw; // udp->sport | udp->dport << 16 as stored, the word at 14 + hl
    uint32_t tt; // tos | ttl << 8 (udp.c:109-110, 119-120; ip6_tos: ip6.h:77-81)
};

// i->flags and i->ttl from frame bytes 12..15 (f0) and 20..23 (f2).
__device__ __forceinline__ uint32_t frame_tos_ttl(bool v4, uint32_t f0, uint32_t f2)
{
    const uint32_t tos = v4 ? f0 >> 24 : (((f0 >> 16) & 0xFu) << 4) | (f0 >> 28);
    const uint32_t ttl = v4 ? (f2 >> 16) & 0xFFu : (f2 >> 8) & 0xFFu; // ttl @8 / hlim @7
    return tos | (ttl << 8);
}

// The parse in ONE load round, on the five chunks of rx_load (or of the RX
// kernel's transposed rx_load_t).  Right for IPv6 and for IPv4 headers of
// 20 <= hl <= 40 bytes; the caller sends every other frame whose header sum
// it needs through frame_hdr_slow.  EXTRA: also the port word and TOS / TTL.
template <bool EXTRA = false>
__device__ __forceinline__ FrameHdr frame_hdr(const u32x4 (&c)[5], uint64_t fa, uint32_t flen)
{
    FrameHdr f;
    f.pw = f.tt = 0u;
    const uint32_t sf = (uint32_t)(fa & 15u);
    // frame bytes 12..23 start in chunk 0 or 1
    const uint32_t o1 = sf + 12u;
    const bool j1 = o1 >= 16u;
    const u32x4 x1 = j1 ? c[1] : c[0], y1 = j1 ? c[2] : c[1];
    uint32_t fw[3];
    win_rot(x1, y1, y1, o1 & 15u, fw);
    f.x = rx_hdr(fw[0], fw[1], fw[2], flen);
    const uint32_t hl = f.x.hl;
    // UDP length / checksum at frame byte 14 + hl + 4: chunk 2, 3 or 4 (20 <= hl <= 40)
    const uint32_t u = sf + 18u + hl;
    const uint32_t ju = min(u >> 4, 4u);
    const u32x4 z4 = {0u, 0u, 0u, 0u};
    const u32x4 xu = ju <= 2u ? c[2] : (ju == 3u ? c[3] : c[4]);
    const u32x4 yu = ju <= 2u ? c[3] : (ju == 3u ? c[4] : z4);
    if constexpr (EXTRA) {
        // the UDP header's first 8 bytes, from frame byte 14 + hl: the same
        // chunks from four bytes earlier (u - 4 >= 34: chunk 2, 3 or 4)
        const uint32_t up = u - 4u;
        const uint32_t jp = up >> 4;
        const u32x4 xp = jp <= 2u ? c[2] : (jp == 3u ? c[3] : c[4]);
        const u32x4 yp = jp <= 2u ? c[3] : (jp == 3u ? c[4] : z4);
        uint32_t uw[2];
        win_rot(xp, yp, yp, up & 15u, uw);
        f.pw = uw[0];
        f.g0 = uw[1];
        f.tt = frame_tos_ttl(f.x.v4, fw[0], fw[2]);
    } else {
        f.g0 = win_bytes(xu, yu, yu, u & 15u, 0);
    }
    // ip_cksum(ip, hl) (ip4.c:110-115) over frame bytes [14, 14 + hl),
    // 20 <= hl <= 40 here (14 + 40 + 15 < 80: inside the five chunks): the
    // header's little-endian words summed header-relative, as csum_oc16 reads
    // them (in_cksum.c:107-120) -- two 20-byte windows rotated out of the
    // chunks, one dot2 per dword, so no address-parity fix.  (Per-chunk byte
    // masks over all five chunks took about twice the VALU.)
    const uint32_t o = sf + 14u;  // header start in the chunk stream: 14..29
    const uint32_t o2 = o + 20u;  // its second 20 bytes: 34..49
    const bool j0 = o >= 16u, j2 = o2 >= 48u;
    uint32_t h0[5], h1[5];
    win_rot(j0 ? c[1] : c[0], j0 ? c[2] : c[1], j0 ? c[3] : c[2], o & 15u, h0);
    win_rot(j2 ? c[3] : c[2], j2 ? c[4] : c[3], j2 ? z4 : c[4], o2 & 15u, h1);
    uint32_t V = 0;
#pragma unroll
    for (int m = 0; m < 5; ++m)
        V = wsum(h0[m], V);
#pragma unroll
    for (int m = 0; m < 5; ++m) // header bytes 20 + 4 m .. 23 + 4 m, if below hl
        V = wsum(hl > 20u + 4u * m ? h1[m] : 0u, V);
    f.ipck = fold_not(V);
    f.f_ip = h0[2] >> 16; // header bytes 10..11, the upper half of header dword 2
    return f;
}

// The same in two load rounds for this lane's frame [fa, fa + flen), any IHL:
// the chunks around frame bytes 12..23 first, then, with the IHL known, the
// UDP fields and the IPv4 header's chunks.  The fallback of frame_hdr.
template <bool EXTRA = false>
__device__ __forceinline__ FrameHdr frame_hdr_slow(uint64_t fa, uint32_t flen, bool valid,
                                                   uint64_t zero)
{
    FrameHdr f;
    f.pw = f.tt = 0u;
    const uint64_t fend = fa + flen;
    const uint64_t a1 = fa + 12u;
    const Win2 w1 = win2_load(a1, fend, valid && flen > 12u, zero);
    uint32_t fw[3]; // frame 12..15, 16..19 = ip 2..5, 20..23 = ip 6..9
    win_rot(w1.x, w1.y, w1.y, (uint32_t)(a1 & 15u), fw);
    f.x = rx_hdr(fw[0], fw[1], fw[2], flen);
    const uint64_t ip = fa + 14u;
    const uint32_t hl = f.x.hl;
    // The UDP length / checksum fields (udp.h:41-46) at ip + hl + 4, and the
    // IPv4 header's chunks, all issued before any is used.
    // (EXTRA: from the port word at ip + hl on; 8 bytes from any phase lie
    // inside the window's two chunks)
    const uint64_t a2 = ip + hl + (EXTRA ? 0u : 4u);
    const Win2 w2 = win2_load(a2, fend, valid && f.x.udp_in, zero);
    const bool hsum = valid && f.x.hdr_in && f.x.v4;
    const uint32_t sip = (uint32_t)(ip & 15u);
    const uint64_t cip = ip & ~15ull;
    const uint32_t nh = hsum ? (sip + hl + 15u) >> 4 : 0u;
    u32x4 hc[kHdrChunks];
#pragma unroll
    for (int k = 0; k < kHdrChunks; ++k)
        hc[k] = load_chunk<false>((uint32_t)k < nh ? cip + 16ull * k : zero);
    // ip_cksum(ip, hl) (ip4.c:110-115): word sum at even addresses; an odd
    // start folds rotl32(V, 8) (the seg path's residue identity; <= 30 words,
    // no wrap).
    uint32_t V = 0;
#pragma unroll
    for (int k = 0; k < kHdrChunks; ++k)
        V += seg_range(hc[k], 16 * k - (int)sip, 0, (int)hl);
    f.ipck = fold_not((ip & 1u) ? __builtin_amdgcn_alignbit(V, V, 24) : V);
    f.f_ip = win_bytes(hc[0], hc[1], hc[2], sip, 2) >> 16; // header bytes 10..11
    if constexpr (EXTRA) {
        uint32_t uw[2];
        win_rot(w2.x, w2.y, w2.y, (uint32_t)(a2 & 15u), uw);
        f.pw = uw[0];
        f.g0 = uw[1];
        f.tt = frame_tos_ttl(f.x.v4, fw[0], fw[2]);
    } else {
        f.g0 = win_bytes(w2.x, w2.y, w2.y, (uint32_t)(a2 & 15u), 0);
    }
    return f;
}

// One 64-chunk row group of 4 rows for the gathered stream (the seg kernel's
// ragged default; 2-row groups measured slower, 128 -> 131 us on the mixed
// ring: profiles/ab_r04_rx_modes.log).
constexpr int kFrameUns = 4;

// A wave's LDS for one tile of 64 frames.
struct FrameLds {
    FlatLds<kFrameUns> f;        // slot table, row marks, prefix sums
    u32x4 stage[64 * kFrameUns]; // (RX: also the header chunks' transpose)
    u32x4 pm[17];                // seg_head's masks
};

// payload_cksum(ip, plen) for the tile's lanes with `need` (the other lanes'
// result means nothing): their packets [ip, ip + plen), and nothing else, as one gathered stream of
// the seg path, the lanes it can't take (header longer than the packet, a
// possible wrap of the odd-start residue) redone exactly by their own lane.
template <bool NT>
__device__ __forceinline__ uint32_t frame_payload_cksum(FrameLds &L, int lane, uint64_t ip,
                                                        uint32_t plen, bool need, uint64_t zero)
{
    using Src = GathSrc<kFrameUns, NT, false>;
    uint32_t r = 0;
    if (__ballot(need)) {
        const FlatTile t = flat_tile_setup<kFrameUns, 1>(L.f, lane, ip, plen, plen, need, 0u);
        bool done = true;
        uint16_t rh = 0;
        r = seg_tile<kFrameUns, WC_KIND_PAYLOAD, NT, false, Src, true>(
            L.f.pre, L.stage, L.pm, lane, ip, 16ull * t.cp + (ip & 15u), plen, need, t.total,
            Src{&L.f, t}, zero, done, rh);
        if (need && !done)
            r = lane_payload_exact<NT>(ip, plen);
        wave_order(); // the tables are rewritten by the next tile
    }
    return r;
}

// --- the RX decision chain and the delivery record ---------------------------
// What the RX verdict kernels (wc_k_rx.hip) and the RX drain kernel
// (wc_k_rxdrain.hip) run on one parsed frame.

// enum wc_rx_verdict (wc_cksum.h)
constexpr uint32_t kRxOk = 0, kRxOkNoCksum = 1, kRxBadIpCksum = 2, kRxBadUdpCksum = 3,
                   kRxShort = 4, kRxFragment = 5, kRxBadVersion = 6, kRxNotUdp = 7,
                   kRxNotIp = 8, kRxTruncated = 9;

__device__ __forceinline__ bool rx_is_drop(uint32_t v)
{
    return v != kRxOk && v != kRxOkNoCksum && v != kRxNotUdp && v != kRxNotIp;
}

struct RxParse {
    uint64_t ip;      // the frame's IP header (frame + 14)
    uint32_t plen;    // payload_cksum length udp_len + hl (need)
    uint32_t verdict; // final unless need
    bool need;        // the UDP checksum must be verified
};

// The reference's decision chain (eth_rx -> ip4_rx / ip6_rx -> udp_rx); bytes
// past the frame only feed decisions that the length checks have made.
__device__ __forceinline__ RxParse rx_decide(uint64_t fa, uint32_t flen, bool valid,
                                             const RxHdr &x, uint32_t g0, uint16_t ipck)
{
    RxParse h{fa + 14u, 0u, kRxTruncated, false};
    const bool v4 = x.v4, v6 = x.v6, frag = x.frag;
    const uint32_t room = x.room, hl = x.hl, proto = x.proto, ip_plen = x.ip_plen;
    const uint32_t ulen = ((g0 & 0xFFu) << 8) | ((g0 >> 8) & 0xFFu);
    const bool ck_zero = (g0 >> 16) == 0u; // udp.c:132
    const uint32_t udp_len = min(ulen, ip_plen); // udp.c:128
    const uint32_t L = udp_len + hl;             // unwrapped; > 65535 is past any frame
    const bool version_ok = x.version_ok, hdr_in = x.hdr_in, udp_in = x.udp_in;
    uint32_t v;
    if (flen < 14u)
        v = kRxTruncated;
    else if (!v4 && !v6)
        v = kRxNotIp;
    else if (room < 1u)
        v = kRxTruncated;
    else if (!version_ok)
        v = kRxBadVersion;
    else if (!hdr_in)
        v = kRxTruncated;
    else if (v4 && ipck != 0)
        v = kRxBadIpCksum;
    else if (frag)
        v = kRxFragment;
    else if (proto != 17u)
        v = kRxNotUdp;
    else if (ip_plen < 8u)
        v = kRxShort;
    else if (!udp_in)
        v = kRxTruncated;
    else if (ck_zero)
        v = kRxOkNoCksum;
    else if (room < max(L, 20u))
        v = kRxTruncated;
    else {
        v = kRxOk;
        h.need = valid;
        h.plen = L;
    }
    h.verdict = v;
    return h;
}

// struct wc_rx_record (wc_cksum.h) of a frame the parse accepts -- kRxOk here
// is "OK unless the UDP sum then fails" --, 16 zero bytes for any other: what
// udp_rx puts into the w_iov (udp.c:101-142, 163-165), as four little-endian
// words.  Every field lies in bytes hdr_in and udp_in have placed inside the
// frame.
__device__ __forceinline__ u32x4 rx_record(const FrameHdr &f, uint32_t verdict)
{
    const uint32_t hl = f.x.hl;
    const uint32_t g0 = f.g0;
    const uint32_t ulen = ((g0 & 0xFFu) << 8) | ((g0 >> 8) & 0xFFu);
    const uint32_t dlen = (min(ulen, f.x.ip_plen) - 8u) & 0xFFFFu; // udp.c:128-129, its wrap
    const bool v4 = f.x.v4;
    u32x4 r;
    r.x = (14u + hl + 8u) | (dlen << 16);                    // data_off, data_len
    r.y = f.pw;                                              // sport, dport as stored
    r.z = (v4 ? 4u : 6u) | (f.tt << 8) | (hl << 24);         // af, tos, ttl, hl
    r.w = v4 ? (26u | (30u << 16)) : (22u | (38u << 16));    // src_off, dst_off
    // (masked, not selected against a zero vector: store data needs registers,
    // and the compiler kept a hoisted {0, 0, 0, 0} live across the whole tile
    // loop -- in scratch, at the 128-VGPR cap)
    const uint32_t take = verdict == kRxOk || verdict == kRxOkNoCksum ? ~0u : 0u;
    return u32x4{r.x & take, r.y & take, r.z & take, r.w & take};
}

// Sixteen zero bytes of store data made where they are stored (see rx_record).
__device__ __forceinline__ u32x4 rx_zero_record()
{
    uint32_t z;
    asm volatile("v_mov_b32 %0, 0" : "=v"(z));
    return u32x4{z, z, z, z};
}

// One record out, as a streaming (nontemporal) store.
__device__ __forceinline__ void rx_rec_store(u32x4 *rec, uint64_t p, const u32x4 &r)
{
    __builtin_nontemporal_store(r, &rec[p]);
}

// rx_parse / rx_parse_slow for the DELIVER kernels: the same decision on a
// parse that also returns the record's fields.
__device__ __forceinline__ RxParse rx_parse_rec(const u32x4 (&c)[5], uint64_t fa, uint32_t flen,
                                                bool valid, bool &slow, u32x4 &rec)
{
    const FrameHdr f = frame_hdr<true>(c, fa, flen);
    slow = valid && f.x.hdr_in && f.x.v4 && (f.x.hl > 40u || f.x.hl < 20u);
    const RxParse h = rx_decide(fa, flen, valid, f.x, f.g0, (uint16_t)f.ipck);
    rec = rx_record(f, slow ? kRxTruncated : h.verdict); // (a slow lane's comes from the slow parse)
    return h;
}

__device__ __forceinline__ RxParse rx_parse_slow_rec(uint64_t fa, uint32_t flen, bool valid,
                                                     uint64_t zero, u32x4 &rec)
{
    const FrameHdr f = frame_hdr_slow<true>(fa, flen, valid, zero);
    const RxParse h = rx_decide(fa, flen, valid, f.x, f.g0, (uint16_t)f.ipck);
    rec = rx_record(f, h.verdict);
    return h;
}

} // namespace
} // namespace wc
