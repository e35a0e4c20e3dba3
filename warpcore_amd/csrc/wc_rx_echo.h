// wc_rx_echo.h -- what the RX echo kernel (wc_k_rxecho.hip) and a host test
// share, each stated once: the length of a socket's
// run under the clamp rule, the prefix of the switched-on runs as the steps of
// a 256-wide scan, entry j -> (socket, list position) by a bounded binary
// search, the record's fields, the classification of an entry, the two
// descriptor forms, the 16-byte window of the payload copy and one lane's share
// of a payload, and the grid size.  Plain C++ (no device builtin), so a host
// program compiles the same lines.  The copy's addressing is
// rr::copy_chunks / rr::copy_dword's (wc_rx_reply.h); their sums are not used.
//
// Reference lines restated (read, not copied):
//   inetd.c:161-169   port 7: sq_concat(&o, &i); w_tx(s, &o) -- every received
//                     iov goes back to its sender, socket after socket
//   udp.c:107-110,141 the iov fields udp_rx fills: address, port, TOS
//   udp.c:189-220     udp_tx writes the headers in front of v->buf
#pragma once

#include <stdint.h>

#include "wc_rx_reply.h"

namespace wc {
namespace re {

// enum wc_rx_echo_status, WC_ECHO_OFF, WC_RX_ECHO_MAX (wc_cksum.h)
constexpr uint32_t kEcho = 0, kNone = 4, kShort = 8, kNoRoom = 9, kStale = 10;
constexpr uint32_t kOff = 0xFFFFu, kMax = 65536u;
constexpr uint32_t kMaxSocks = 254u; // WC_RX_DEMUX_MAX_SOCKS: runs 0 .. 253 of d_start[256]
constexpr uint32_t kRuns = 256u;     // the scan's width (runs at and past ns have length 0)
constexpr uint32_t kScanSteps = 8u;  // log2(kRuns)
constexpr uint32_t kWave = 64u;      // entries per workgroup: one wave, lane l = entry l
constexpr uint32_t kGroup = 16u;     // lanes that move one payload together
constexpr uint32_t kUnroll = 6u;     // chunks a lane loads before it stores: 16 * 6 * 16 B >= an MTU payload

WC_HD bool is_skip(uint32_t st)
{
    return st == kShort || st == kNoRoom || st == kStale;
}

// Socket s's run is [s0, s1) = [start[s], start[s + 1]); it counts only if the
// socket is switched on (a map value <= 255) and s0 <= s1 <= n.
WC_HD uint64_t run_len(uint64_t s0, uint64_t s1, uint64_t n, uint32_t map)
{
    return map <= 255u && s0 <= s1 && s1 <= n ? s1 - s0 : 0ull;
}

// One element of one step (d = 1, 2, 4 ... 128) of the inclusive scan over
// kRuns lengths: out[t] = in[t] + in[t - d].  After kScanSteps steps, each from
// the buffer the step before wrote, inc[t] = the total of runs 0 .. t; the
// echo count E is inc[kRuns - 1] (at most 254 * 2^32: no wrap).
WC_HD void scan_step(const uint64_t *in, uint64_t *out, uint32_t t, uint32_t d)
{
    out[t] = in[t] + (t >= d ? in[t - d] : 0ull);
}

// Entry j < E lies in the run of the first socket s with inc[s] > j: at most
// kScanSteps halvings of [0, ns), ns <= 254.  pos: its place in that run.
struct Where {
    uint32_t s;
    uint64_t pos;
};

WC_HD Where where_of(const uint64_t *inc, uint32_t ns, uint64_t j)
{
    uint32_t lo = 0u, hi = ns;
    for (uint32_t k = 0; k < kScanSteps; ++k) {
        if (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (inc[mid] <= j)
                lo = mid + 1u;
            else
                hi = mid;
        }
    }
    return Where{lo, j - (lo ? inc[lo - 1u] : 0ull)};
}

// struct wc_rx_record as its four little-endian dwords.
struct Rec {
    uint32_t data_off, data_len, sport, af, tos, hl, src_off;
};

WC_HD Rec rec_of(uint32_t x, uint32_t y, uint32_t z, uint32_t w)
{
    return Rec{x & 0xFFFFu, x >> 16, y & 0xFFFFu, z & 0xFFu, (z >> 8) & 0xFFu, z >> 24, w & 0xFFFFu};
}

WC_HD uint32_t hl_tx(uint32_t af)
{
    return af == 4u ? 20u : 40u;
}

// The status of an entry j < min(E, m); the first rule that holds names it.
//   STALE    the list index is not below n, the record's af is not 4 / 6, or
//            the record is none that a delivery writes for a frame of flen
//            bytes: hl below the built header's, data_off not 14 + hl + 8, or
//            the source address not inside the frame.  (Such a record would
//            move an address read or the in-place frame start off the frame.)
//   SHORT    data_off + data_len > flen
//   NO_ROOM  copy mode and 14 + hl_tx + 8 + data_len > out_slot_bytes
WC_HD uint32_t classify(bool idx_in, const Rec &r, uint32_t flen, bool copy, uint32_t out_slot_bytes)
{
    if (!idx_in || (r.af != 4u && r.af != 6u))
        return kStale;
    const uint32_t h = hl_tx(r.af);
    if (r.hl < h || r.data_off != 14u + r.hl + 8u || r.src_off + (r.af == 4u ? 4u : 16u) > flen)
        return kStale;
    if (r.data_off + r.data_len > flen)
        return kShort;
    if (copy && 14u + h + 8u + r.data_len > out_slot_bytes)
        return kNoRoom;
    return kEcho;
}

// struct wc_tx_desc as two dwords: data_len | ip_id << 16, sock | tos << 8 |
// dst << 16.  The inert form fails the build's check 3 (14 + hl + 8 + 0xFFFF >
// 65535) whatever socket 0 is.
WC_HD void desc_words(const Rec &r, uint32_t ip_id, uint32_t sock, uint32_t j, uint32_t (&d)[2])
{
    d[0] = r.data_len | ((ip_id & 0xFFFFu) << 16);
    d[1] = (sock & 0xFFu) | (r.tos << 8) | (j << 16);
}

WC_HD void inert_words(uint32_t j, uint32_t (&d)[2])
{
    d[0] = 0xFFFFu;
    d[1] = j << 16;
}

// struct wc_tx_dst as six dwords: addr (IPv4: one dword and twelve zero bytes),
// then dmac | port << 16 in the last two.  mac0 / mac1: frame bytes 6..9 and
// 10..11.
WC_HD void dst_words(const Rec &r, const uint32_t (&src)[4], uint32_t mac0, uint32_t mac1,
                     uint32_t (&t)[6])
{
    const bool v4 = r.af == 4u;
    t[0] = src[0];
    t[1] = v4 ? 0u : src[1];
    t[2] = v4 ? 0u : src[2];
    t[3] = v4 ? 0u : src[3];
    t[4] = mac0;
    t[5] = (mac1 & 0xFFFFu) | (r.sport << 16);
}

// Sixteen bytes from byte sh (0 .. 15) of the 32 bytes X:Y on, in two select
// levels and a funnel shift (the window of rr::copy_chunk).
WC_HD rr::Quad window(const rr::Quad &X, const rr::Quad &Y, uint32_t sh)
{
    const bool q1 = sh & 4u, q2 = sh & 8u;
    const uint32_t bs = 8u * (sh & 3u);
    const uint32_t e0 = q1 ? X.y : X.x, e1 = q1 ? X.z : X.y, e2 = q1 ? X.w : X.z,
                   e3 = q1 ? Y.x : X.w, e4 = q1 ? Y.y : Y.x, e5 = q1 ? Y.z : Y.y,
                   e6 = q1 ? Y.w : Y.z;
    const uint32_t d0 = q2 ? e2 : e0, d1 = q2 ? e3 : e1, d2 = q2 ? e4 : e2, d3 = q2 ? e5 : e3,
                   d4 = q2 ? e6 : e4;
    if (bs == 0u)
        return rr::Quad{d0, d1, d2, d3};
    const uint32_t ls = 32u - bs;
    return rr::Quad{(d0 >> bs) | (d1 << ls), (d1 >> bs) | (d2 << ls), (d2 >> bs) | (d3 << ls),
                    (d3 >> bs) | (d4 << ls)};
}

// Lane g (< kGroup) of the group's share of one payload: the len bytes at sa go
// to dd.  The aligned 16-byte destination chunks that lie wholly inside [dd, dd
// + len) (rr::copy_chunks) are dealt round-robin to the lanes; a lane loads the
// source chunks of kUnroll of its destination chunks -- each from the one or two
// aligned source chunks that hold it, all of which overlap [sa, sa + len) --
// before it stores the first, so that a whole MTU payload is in flight at once.
// The at most four dwords in front of the whole chunks and four behind them
// (nine in all where there is no whole chunk) go one per lane through
// rr::copy_dword: whole dwords whole, the two ends as 2-byte / byte stores at
// natural alignment.  No byte outside [dd, dd + len) is written.  Any source
// phase with any destination phase.  Mem: ld32 / st8 / st16 / st32 / ld128 /
// st128.
template <class Mem>
WC_HD void copy_lane(const Mem &m, uint64_t sa, uint64_t dd, uint32_t len, uint32_t g)
{
    const rr::Chunks ch = rr::copy_chunks(dd, len);
    const uint64_t s0 = sa - (dd & 15u), d0 = dd & ~15ull; // chunk c: from s0 + 16 c to d0 + 16 c
    const uint32_t sh = (uint32_t)(s0 & 15u);              // the same for every chunk
    for (uint32_t c = ch.c0 + g; c < ch.c1; c += kGroup * kUnroll) {
        rr::Quad X[kUnroll], Y[kUnroll];
#if defined(__clang__)
#pragma unroll
#endif
        for (uint32_t u = 0; u < kUnroll; ++u) {
            const uint32_t cu = c + kGroup * u;
            X[u] = Y[u] = rr::Quad{0u, 0u, 0u, 0u};
            if (cu < ch.c1) {
                const uint64_t a = (s0 + 16ull * cu) & ~15ull;
                X[u] = m.ld128(a);
                if (sh != 0u)
                    Y[u] = m.ld128(a + 16u);
            }
        }
#if defined(__clang__)
#pragma unroll
#endif
        for (uint32_t u = 0; u < kUnroll; ++u) {
            const uint32_t cu = c + kGroup * u;
            if (cu < ch.c1)
                m.st128(d0 + 16ull * cu, window(X[u], Y[u], sh));
        }
    }
    const uint32_t nd = rr::copy_dwords(dd, len);
    const uint32_t i = g < ch.i0 ? g : ch.i1 + (g - ch.i0);
    if (i < nd)
        (void)rr::copy_dword(m, sa, dd, len, i);
}

// One one-wave workgroup per kWave entries; m = 0 still takes one, for *count.
WC_HD uint32_t grid_of(uint32_t m)
{
    return m ? (m + kWave - 1u) / kWave : 1u;
}

} // namespace re
} // namespace wc
