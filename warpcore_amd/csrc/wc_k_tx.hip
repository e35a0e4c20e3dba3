// wc_k_tx.hip -- the TX seal kernel on gfx950: for every Ethernet frame of a
// batch, the two checksums the reference's TX path computes and stores
// (INTEGRATION.md section 3), computed on the device from
// the frame bytes alone and stored raw into the frame.
//
// Reference stores restated (read, not copied):
//   mk_ip4_hdr  /root/reference/lib/src/ip4.c:184-186   ip->cksum = 0, then
//               ip->cksum = ip_cksum(ip, hl)
//   udp_tx      /root/reference/lib/src/udp.c:209-213   udp->cksum = 0, then
//               (unless the socket sends zero checksums) udp->cksum =
//               payload_cksum(ip, hl + udp_len), a computed 0 stored as 0
// The field reads and their order are the RX chain's (wc_k_rx.hip); the codes
// are enum wc_tx_status (wc_cksum.h).  The header parse and the gathered
// stream are the RX kernel's own code (wc_rx_hdr.h); this file keeps the
// decision chain (tx_decide) and the stores.
//
// One wave per tile of 64 frames (lane l = frame l), one-shot grid, the RX
// kernel's EARLY structure:
//   1. the frame's first five aligned chunks, each only where it overlaps the
//      frame: every header field, the IPv4 header's sum (up to 40 bytes) and
//      the UDP length (frame_hdr) -- the status is final here;
//   2. the frames whose UDP checksum is computed go through the gathered
//      stream of the seg path (frame_payload_cksum: seg_tile over [ip, ip +
//      hl + udp_len), the lanes it can't take redone by lane_payload_exact);
//      IPv4 headers longer than 40 bytes take a per-lane path of their own
//      (tx_parse_slow, frame_hdr_slow);
//   3. with every load of the tile's frames back (s_waitcnt vmcnt(0)), each
//      lane stores its one or two fields: one 2-byte store at an even address,
//      two byte stores at an odd one.
// Both sums are taken over the bytes as they lie, whatever the two fields
// hold; the field's word is then taken out of the folded result by a
// one's-complement subtraction (oc16_without).  No byte outside a frame is
// read or written, and no byte of a frame but its two fields is written.
// Bytes of neighbouring frames that share a 16-byte chunk with this one
// cancel out of the stream's prefix differences (each loaded chunk is used
// from one register copy), so another wave storing its own frame's fields
// meanwhile changes nothing here: frames of one call must not overlap.
// Roofline: HBM, the sealed frames' bytes once.
#include "wc_rx_hdr.h"

namespace wc {
namespace {

// enum wc_tx_status (wc_cksum.h)
constexpr uint32_t kTxSealed = 0, kTxSealedZeroUdp = 1, kTxIpOnly = 2, kTxNotUdp = 3,
                   kTxNotIp = 4, kTxBadVersion = 5, kTxMalformed = 6, kTxTruncated = 7;

struct TxParse {
    uint32_t status;
    uint32_t hl;
    uint32_t plen;        // payload_cksum length hl + udp_len (need)
    uint32_t ipck;        // ip_cksum(ip, hl) of the header as loaded (ipst)
    uint32_t f_ip, f_udp; // ip->cksum, udp->cksum as loaded (native words)
    bool ipst;            // the IPv4 header checksum is stored
    bool udpst;           // udp->cksum is stored (0, or the computed sum)
    bool need;            // the UDP checksum is computed
};

// ~fold(S - f) from r = ~fold(S): S the reference's uint32 accumulator over
// bytes that include the native word f (no wrap, S - f > 0 -- the version
// byte, or the pseudo-header's protocol, is in it).  fold (csum_oc16_reduce,
// in_cksum.c:74-80) maps a positive sum to its residue mod 0xFFFF in
// [1, 0xFFFF]; ~r is fold(S) and ~f == -f, so their sum is positive and
// congruent to S - f: its fold is fold(S - f) itself, 0xFFFF (never 0) where
// the residue is 0 -- the reference's result for f == 0x0000 and 0xFFFF alike.
__device__ __forceinline__ uint32_t oc16_without(uint32_t r, uint32_t f)
{
    return fold_not((~r & 0xFFFFu) + (~f & 0xFFFFu));
}

// The seal's decision chain (wc_cksum.h, enum wc_tx_status): the RX chain's
// order; bytes past the frame only feed decisions that the length checks have
// made.
__device__ __forceinline__ TxParse tx_decide(uint32_t flen, bool valid, const RxHdr &x, uint32_t g0,
                                             uint32_t ipck, uint32_t f_ip, bool zero_udp)
{
    TxParse h{kTxTruncated, x.hl, 0u, ipck, f_ip, g0 >> 16, false, false, false};
    const uint32_t room = x.room, hl = x.hl;
    const uint32_t ulen = ((g0 & 0xFFu) << 8) | ((g0 >> 8) & 0xFFu);
    const uint32_t udp_len = min(ulen, x.ip_plen); // udp.c:128
    const uint32_t L = hl + udp_len;               // unwrapped; > 65535 is past any frame
    uint32_t s;
    if (flen < 14u)
        s = kTxTruncated;
    else if (!x.v4 && !x.v6)
        s = kTxNotIp;
    else if (room < 1u)
        s = kTxTruncated;
    else if (!x.version_ok)
        s = kTxBadVersion;
    else if (x.v4 && hl < 20u)
        s = kTxMalformed;
    else if (room < hl)
        s = kTxTruncated;
    else if (x.proto != 17u || x.frag) {
        s = x.v4 ? kTxIpOnly : kTxNotUdp;
        h.ipst = valid && x.v4;
    } else if (x.ip_plen < 8u)
        s = kTxMalformed;
    else if (room < hl + 8u)
        s = kTxTruncated;
    else if (udp_len < 8u)
        s = kTxMalformed;
    else if (zero_udp) {
        s = kTxSealedZeroUdp;
        h.ipst = valid && x.v4;
        h.udpst = valid;
    } else if (room < L)
        s = kTxTruncated;
    else {
        s = kTxSealed;
        h.ipst = valid && x.v4;
        h.udpst = valid;
        h.need = valid;
        h.plen = L;
    }
    h.status = s;
    return h;
}

// The one-round parse (frame_hdr, wc_rx_hdr.h) and the decision on it.  `slow`:
// an IPv4 header longer than 40 bytes is not inside the five chunks
// (tx_parse_slow).  Unlike the RX kernel's rx_parse, IHL < 5 does not ask for
// it: tx_decide rules such a header MALFORMED without looking at its sum.
__device__ __forceinline__ TxParse tx_parse(const u32x4 (&c)[5], uint64_t fa, uint32_t flen,
                                            bool valid, bool zero_udp, bool &slow)
{
    const FrameHdr f = frame_hdr(c, fa, flen);
    slow = valid && f.x.hdr_in && f.x.v4 && f.x.hl > 40u;
    return tx_decide(flen, valid, f.x, f.g0, f.ipck, f.f_ip, zero_udp);
}

// The fallback of tx_parse: two load rounds, any IHL (frame_hdr_slow).
__device__ __forceinline__ TxParse tx_parse_slow(uint64_t fa, uint32_t flen, bool valid,
                                                 bool zero_udp, uint64_t zero)
{
    const FrameHdr f = frame_hdr_slow(fa, flen, valid, zero);
    return tx_decide(flen, valid, f.x, f.g0, f.ipck, f.f_ip, zero_udp);
}

// A native uint16 stored raw at any address parity, as the reference's
// `ip->cksum = ...` / `udp->cksum = ...` leave it in memory.
__device__ __forceinline__ void store_raw16(uint64_t a, uint32_t v)
{
    if (a & 1u) {
        gst8_ptr p = (gst8_ptr)(uintptr_t)a;
        p[0] = (uint8_t)v;
        p[1] = (uint8_t)(v >> 8);
    } else {
        *(gst16_ptr)(uintptr_t)a = (uint16_t)v;
    }
}

constexpr int kTxSpan = 15; // XCD super-blocks of 2^15 tiles, as the RX kernel's

// One-wave workgroups and 4 waves per SIMD, as k_rx_verdict's EARLY mode.
// STORE = false (WC_TX_NO_STORE, the host call): the frames are only read.
template <bool NT, bool STORE>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4)))
k_tx_seal(uint8_t *base, const uint64_t *__restrict__ offs,
          const uint16_t *__restrict__ flens, uint64_t n, uint32_t zero_udp_flag,
          uint8_t *__restrict__ status, uint16_t *__restrict__ out_ip,
          uint16_t *__restrict__ out_udp, unsigned long long *__restrict__ errors)
{
    __shared__ FrameLds L;

    const int lane = threadIdx.x & 63;
    const bool zero_udp = zero_udp_flag != 0u; // wave-uniform
    seg_init_masks(L.pm, lane); // read after the first row group's wave_order
    const uint64_t ntiles = (n + 63) / 64;
    const uint64_t nwaves = gridDim.x;
    uint64_t tile = xcd_block(kTxSpan << 8);
    uint32_t nerr = 0;
    const uint64_t zero = (uint64_t)(uintptr_t)&kZeroChunk;

    uint64_t off_n;
    uint32_t flen_n;
    meta_load(offs, flens, tile * 64 + lane, n, off_n, flen_n);

    for (; tile < ntiles; tile += nwaves) {
        const uint64_t p = tile * 64 + lane;
        const bool valid = p < n;
        const uint64_t fa = (uint64_t)(uintptr_t)base + off_n;
        const uint32_t flen = flen_n;
        meta_load(offs, flens, (tile + nwaves) * 64 + lane, n, off_n, flen_n);

        u32x4 c[5];
        rx_load(fa, flen, valid, zero, c);
        const uint64_t ip = fa + 14u;
        bool slow = false;
        TxParse h = tx_parse(c, fa, flen, valid, zero_udp, slow);
        // payload_cksum(ip, plen) of the bytes as loaded (need)
        uint32_t r = frame_payload_cksum<NT>(L, lane, ip, h.plen, h.need && !slow, zero);
        if (__ballot(slow)) { // IPv4 headers with more than 20 B of options
            const TxParse hs = tx_parse_slow(fa, flen, slow, zero_udp, zero);
            if (slow) {
                h = hs;
                if (hs.need)
                    r = lane_payload_exact<NT>(ip, hs.plen);
            }
        }
        const uint32_t ipv = h.ipst ? oc16_without(h.ipck, h.f_ip) : 0u;
        const uint32_t udpv = h.need ? oc16_without(r, h.f_udp) : 0u; // (a computed 0 stays 0)
        if constexpr (STORE) {
            // Every load of this tile's frames has returned before the first
            // field is written.
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (h.ipst)
                store_raw16(ip + 10u, ipv);
            if (h.udpst)
                store_raw16(ip + h.hl + 6u, udpv);
        }
        if (valid) {
            status[p] = (uint8_t)h.status;
            if (out_ip)
                out_ip[p] = (uint16_t)ipv;
            if (out_udp)
                out_udp[p] = (uint16_t)udpv;
        }
        nerr += valid && h.status >= kTxBadVersion;
    }
    if (errors) {
        nerr = group_sum<64>(nerr);
        if (lane == 0 && nerr)
            atomicAdd(errors, (unsigned long long)nerr);
    }
}

} // namespace

template <bool NT, bool STORE>
static hipError_t launch_tx_one(void *base, const uint64_t *offs, const uint16_t *flens,
                                uint64_t n, uint32_t zero_udp, uint8_t *status, uint16_t *out_ip,
                                uint16_t *out_udp, uint64_t *errors, int grid, hipStream_t st)
{
    hipLaunchKernelGGL((k_tx_seal<NT, STORE>), dim3(grid), dim3(64), 0, st, (uint8_t *)base, offs,
                       flens, n, zero_udp, status, out_ip, out_udp, (unsigned long long *)errors);
    return hipGetLastError();
}

hipError_t launch_tx_seal(void *base, const uint64_t *offs, const uint16_t *flens, uint64_t n,
                          uint32_t flags, uint8_t *status, uint16_t *out_ip, uint16_t *out_udp,
                          uint64_t *errors, bool nt, hipStream_t st)
{
    const int grid = tile_grid(n);
    const uint32_t zu = (flags & kTxZeroUdp) ? 1u : 0u;
    const bool store = !(flags & kTxNoStore);
#define WC_TX(N, S)                                                            \
    if (nt == N && store == S)                                                 \
        return launch_tx_one<N, S>(base, offs, flens, n, zu, status, out_ip, out_udp, errors,  \
                                   grid, st);
    WC_TX(true, true) WC_TX(true, false) WC_TX(false, true) WC_TX(false, false)
#undef WC_TX
    return hipErrorInvalidValue; // (every combination is listed above)
}

} // namespace wc
