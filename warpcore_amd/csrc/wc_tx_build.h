// wc_tx_build.h -- what the TX build kernel (wc_k_txbuild.hip) and the host
// call (wc_tx_build_host, wc_rt_tx.cpp) share about one frame, each stated
// once: the table entries as little-endian dwords, the
// check chain, the 42 or 62 header bytes as frame-relative dwords, and the
// stores of those bytes at any 4-byte phase.  The RX reply and RX neighbour
// paths (wc_rx_reply.h, wc_rx_neigh.h) take the byte swap, the folds, the
// 14-byte shift (shift14) and the stores (store_words) from here.  Plain C++
// (no device builtin), so the host call and a host test compile the same lines.
//
// Reference stores restated (read, not copied):
//   mk_eth_hdr  /root/reference/lib/src/eth.h:89-109    dst, src, type
//   mk_ip4_hdr  /root/reference/lib/src/ip4.c:153-189   vhl, tos (| ECT0), len,
//               id (unswapped), DF, ttl 0xff, p, src, dst, cksum
//   mk_ip6_hdr  /root/reference/lib/src/ip6.c:127-161   vtcecnfl (the ORs on a
//               zeroed word), len, next_hdr, hlim 0xff, src, dst
//   udp_tx      /root/reference/lib/src/udp.c:189-220   sport, dport, len, cksum
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__HIP__)
#define WC_HD __host__ __device__ __forceinline__
#else
#define WC_HD inline
#endif

namespace wc {
namespace txb {

// enum wc_tx_status (wc_cksum.h): the codes a build gives
constexpr uint32_t kSealed = 0, kSealedZeroUdp = 1, kMalformed = 6, kTruncated = 7;
constexpr uint32_t kSockConnected = 1, kSockEcn = 2; // WC_TX_SOCK_*
constexpr uint32_t kSockWords = 13, kDstWords = 6;   // struct wc_tx_sock / wc_tx_dst in dwords

// struct wc_tx_sock as dwords: w[0] = af | flags << 8 | lport << 16, w[1] =
// rport | smac[0..1] << 16, w[2] = smac[2..5], w[3] = dmac[0..3], w[4] =
// dmac[4..5] | pad << 16, w[5..8] = laddr, w[9..12] = raddr.
// struct wc_tx_dst: t[0..3] = addr, t[4] = dmac[0..3], t[5] = dmac[4..5] |
// port << 16.
// struct wc_tx_desc: d[0] = data_len | ip_id << 16, d[1] = sock | tos << 8 |
// dst << 16.
struct Desc {
    uint32_t data_len, ip_id, sock, tos, dst;
};

WC_HD Desc desc_of(uint32_t d0, uint32_t d1)
{
    return Desc{d0 & 0xFFFFu, d0 >> 16, d1 & 0xFFu, (d1 >> 8) & 0xFFu, d1 >> 16};
}

WC_HD uint32_t bswap16(uint32_t x)
{
    return ((x & 0xFFu) << 8) | ((x >> 8) & 0xFFu);
}

// The two little-endian 16-bit words of a dword, summed.
WC_HD uint32_t words(uint32_t x)
{
    return (x & 0xFFFFu) + (x >> 16);
}

// A sum below 2^32 folded to 16 bits, and in_cksum.c:74-80 on it.
WC_HD uint32_t fold16(uint32_t s)
{
    s = (s & 0xFFFFu) + (s >> 16);
    s = (s & 0xFFFFu) + (s >> 16);
    return s;
}

WC_HD uint32_t fold_not16(uint32_t s)
{
    return ~fold16(s) & 0xFFFFu;
}

// N dwords that follow an Ethernet header, as frame-relative dwords: they lie
// 14 bytes into the frame, behind dst, src (h[0 .. 2], the caller's) and the
// EtherType as stored.  h[3 + N] holds the last two bytes in its low half.
template <int N>
WC_HD void shift14(uint32_t etype, const uint32_t (&ip)[N], uint32_t (&h)[N + 4])
{
    h[3] = etype | (ip[0] << 16);
#if defined(__clang__)
#pragma unroll
#endif
    for (int k = 1; k < N; ++k)
        h[3 + k] = (ip[k - 1] >> 16) | (ip[k] << 16);
    h[3 + N] = ip[N - 1] >> 16;
}

// The check chain (wc_cksum.h, "TX build"), in its order.  sock_in / dst_in:
// the descriptor's indices lie inside the tables (w0 is read only then);
// hl / hb / flen are set for every entry whose af is 4 or 6.
struct Decide {
    uint32_t status;
    bool v4, connected, ecn;
    uint32_t hl, hb, flen; // IP header, all headers (14 + hl + 8), the frame
};

WC_HD Decide decide(bool sock_in, uint32_t w0, bool dst_in, uint32_t data_len, uint32_t slot_bytes,
                    bool zero_udp)
{
    Decide x;
    const uint32_t af = w0 & 0xFFu, fl = (w0 >> 8) & 0xFFu;
    x.v4 = af == 4u;
    x.connected = fl & kSockConnected;
    x.ecn = fl & kSockEcn;
    x.hl = x.v4 ? 20u : 40u;
    x.hb = 14u + x.hl + 8u;
    x.flen = x.hb + data_len;
    if (!sock_in || (af != 4u && af != 6u))
        x.status = kMalformed;
    else if (!x.connected && !dst_in)
        x.status = kMalformed;
    else if (x.flen > 65535u)
        x.status = kMalformed;
    else if (x.flen > slot_bytes)
        x.status = kTruncated;
    else
        x.status = zero_udp ? kSealedZeroUdp : kSealed;
    return x;
}

// The headers of one frame as little-endian dwords from the frame's first
// byte: h[0 .. 10] hold the 42 bytes of an IPv4 frame (h[10]: its low half),
// h[0 .. 15] the 62 of an IPv6 one (h[15]: its low half).
struct Hdr {
    uint32_t h[16];
    uint32_t ip_hdr, udp; // the two checksum values as stored (0: none)
};

// w / t: the socket and (for an unconnected one) destination entry; pay: the
// folded sum of the payload's words from its first byte on, ~ip_cksum(payload)
// (0 with zero_udp or no payload).  sums = false (the host call): both
// checksum fields are left 0.
//
// The UDP sum is the reference's (in_cksum.c:146-164): proto << 8 (IPv4) or
// next_hdr << 24 (IPv6), the address words, the length word, then the UDP
// header and payload words.  Nothing wraps: 17 << 24 plus 16 address words,
// 4 more header words and one folded payload word stays below 2^29; the
// reference's own accumulator, which adds the payload's <= 32747 words
// unfolded, stays below 2^32 too (17 << 24 + 32800 * 0xFFFF < 0x91000000), so
// both are positive numbers with the same residue mod 0xFFFF and fold alike.
WC_HD Hdr headers(const Decide &x, const Desc &d, const uint32_t (&w)[kSockWords],
                  const uint32_t (&t)[kDstWords], uint32_t pay, bool zero_udp, bool sums)
{
    const bool c = x.connected, v4 = x.v4;
    const uint32_t dm0 = c ? w[3] : t[4], dm1 = (c ? w[4] : t[5]) & 0xFFFFu;
    const uint32_t dport = c ? w[1] & 0xFFFFu : t[5] >> 16;
    const uint32_t s0 = w[5], s1 = w[6], s2 = w[7], s3 = w[8];
    const uint32_t d0 = c ? w[9] : t[0], d1 = c ? w[10] : t[1], d2 = c ? w[11] : t[2],
                   d3 = c ? w[12] : t[3];
    const uint32_t pw = (w[0] >> 16) | (dport << 16);      // udp->sport, dport (udp.c:206-207)
    const uint32_t ulen = bswap16(8u + d.data_len);        // udp->len, ip6->len (udp.c:208)
    const bool no_ecn = (d.tos & 3u) == 0u;
    // IPv4 header dwords (ip4.c:156-182), checksum field 0
    const uint32_t tos4 = d.tos | (no_ecn && x.ecn ? 2u : 0u);
    const uint32_t a0 = 0x45u | (tos4 << 8) | (bswap16(28u + d.data_len) << 16);
    const uint32_t a1 = d.ip_id | (0x0040u << 16); // id as stored, then DF
    const uint32_t a2 = 0xFFu | (17u << 8);        // ttl, protocol
    // IPv6 first word (ip6.c:132-138) and len / next_hdr / hlim
    const uint32_t b0 = no_ecn ? 0x60u | (x.ecn ? 0x20u << 16 : 0u)
                               : 0x60u | (d.tos >> 4) | ((d.tos & 0x0Fu) << 12);
    const uint32_t b1 = ulen | (17u << 16) | (0xFFu << 24);

    Hdr r;
    r.ip_hdr = r.udp = 0u;
    if (sums) {
        if (v4) // ip_cksum(ip, 20) with the field 0 (ip4.c:185-186)
            r.ip_hdr = fold_not16(words(a0) + words(a1) + words(a2) + words(s0) + words(d0));
        if (!zero_udp) {
            uint32_t S = v4 ? (17u << 8) + words(s0) + words(d0)
                            : (17u << 24) + words(s0) + words(s1) + words(s2) + words(s3) +
                                  words(d0) + words(d1) + words(d2) + words(d3);
            S += ulen;                    // the pseudo-header's length word
            S += words(pw) + ulen + pay;  // the UDP header (field 0) and the payload
            r.udp = fold_not16(S);        // a computed 0 stays 0 (udp.c:213)
        }
    }
    const uint32_t uw = ulen | (r.udp << 16);
    // The IP and UDP dwords from the IP header's first byte on ...
    const uint32_t i0 = v4 ? a0 : b0, i1 = v4 ? a1 : b1, i2 = v4 ? a2 | (r.ip_hdr << 16) : s0,
                   i3 = v4 ? s0 : s1, i4 = v4 ? d0 : s2, i5 = v4 ? pw : s3, i6 = v4 ? uw : d0;
    const uint32_t ip[12] = {i0, i1, i2, i3, i4, i5, i6, d1, d2, d3, pw, uw};
    // ... lie 14 bytes into the frame: behind dst, src (eth.h:93-105) and type.
    r.h[0] = dm0;
    r.h[1] = dm1 | (w[1] & 0xFFFF0000u);
    r.h[2] = w[2];
    shift14(v4 ? 0x0008u : 0xDD86u, ip, r.h);
    return r;
}

// The stores of h's first 4 N - 2 bytes at address fa (a byte-granular
// integer), N = NA where short_form holds and NB otherwise -- 42 or 62 header
// bytes for <11, 16>, a fixed length where NA == NB (the choice then folds at
// compile time): the bytes are shifted to fa's 4-byte phase and written as
// aligned dwords, the ends as byte / 2-byte stores at their natural alignment,
// so no byte outside [fa, fa + 4 N - 2) is written at any phase.  Mem: st8 /
// st16 / st32(address, value).  The length is 2 mod 4, which fixes the shape
// of the two ends per phase.  One statement for both lengths, not one call per
// length: the lanes of a TX build tile differ in short_form, and two calls
// would run one after the other in a mixed tile.
template <int NA, int NB, class Mem>
WC_HD void store_words(const Mem &m, uint64_t fa, bool short_form, const uint32_t (&h)[NB])
{
    static_assert(2 <= NA && NA <= NB, "the short form is a prefix of the long one");
    const bool sf = NA == NB || short_form;
    const uint32_t p = (uint32_t)(fa & 3u), sh = 8u * p;
    const uint64_t b = fa - p; // aligned dword j lies at b + 4 j and holds frame bytes [4 j - p, + 4)
    // Aligned dword j, 1 <= j < NB, computed where it is stored: values, not
    // elements of a shifted array, and every index a constant (a select between
    // two array elements becomes a dynamic index, and a 64-bit funnel of two
    // neighbours one 8-byte load of the array: either puts h in scratch).
    const uint32_t rs = (32u - sh) & 31u, keep = p ? 0xFFFFFFFFu : 0u;
    auto al = [&](int j) { return (h[j] << sh) | ((h[j - 1] >> rs) & keep); };
    // the first dword: whole at phase 0, else its upper 4 - p bytes
    if (p == 0u) {
        m.st32(b, h[0]);
    } else if (p == 2u) {
        m.st16(fa, h[0] & 0xFFFFu);
    } else {
        m.st8(fa, h[0] & 0xFFu);
        if (p == 1u)
            m.st16(fa + 1u, (h[0] >> 8) & 0xFFFFu);
    }
    // whole dwords: 1 .. NA - 2 always; NA - 1 from phase 2 on (p + 4 NA - 2 >=
    // 4 NA) or for the long form; NA .. NB - 2 for the long form; NB - 1 for the
    // long form from phase 2 on
#if defined(__clang__)
#pragma unroll
#endif
    for (int j = 1; j < NA - 1; ++j)
        m.st32(b + 4u * j, al(j));
    const uint32_t aa = al(NA - 1), ab = al(NB - 1);
    if (!sf || p >= 2u)
        m.st32(b + 4u * (NA - 1), aa);
    if (!sf) {
#if defined(__clang__)
#pragma unroll
#endif
        for (int j = NA; j < NB - 1; ++j)
            m.st32(b + 4u * j, al(j));
        if (p >= 2u)
            m.st32(b + 4u * (NB - 1), ab);
    }
    // the last dword's first (p + 2) & 3 bytes: dword (p + 4 N - 2) >> 2, of
    // which only phases 0, 1 (dword N - 1) and 3 (dword N: the last byte) have
    // any
    const uint32_t m4 = sf ? 0xFFFFFFFFu : 0u;
    const uint32_t hi = (h[NA - 1] & m4) | (h[NB - 1] & ~m4); // the last two bytes (no select
                                                              // between elements: see above)
    const uint32_t tl = p >= 2u ? (hi >> 8) & 0xFFu : (sf ? aa : ab);
    const uint32_t je = (sf ? NA - 1u : NB - 1u) + (p >= 2u ? 1u : 0u);
    const uint64_t ta = b + 4u * je;
    if (p == 0u) {
        m.st16(ta, tl & 0xFFFFu);
    } else if (p == 1u) {
        m.st16(ta, tl & 0xFFFFu);
        m.st8(ta + 2u, (tl >> 16) & 0xFFu);
    } else if (p == 3u) {
        m.st8(ta, tl & 0xFFu);
    }
}

// The 42 (v4) or 62 header bytes of Hdr::h, a built frame's or a reply's.
template <class Mem>
WC_HD void store_headers(const Mem &m, uint64_t fa, bool v4, const uint32_t (&h)[16])
{
    store_words<11, 16>(m, fa, v4, h);
}

} // namespace txb
} // namespace wc
