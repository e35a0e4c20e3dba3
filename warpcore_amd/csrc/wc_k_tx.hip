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
// The field reads and their order are the RX chain's (wc_k_rx.hip, the header
// view of wc_rx_hdr.h); the codes are enum wc_tx_status (wc_cksum.h).
//
// One wave per tile of 64 frames (lane l = frame l), one-shot grid, the RX
// kernel's EARLY structure:
//   1. the frame's first five aligned chunks, each only where it overlaps the
//      frame: every header field, the IPv4 header's sum (up to 40 bytes) and
//      the UDP length -- the status is final here;
//   2. the frames whose UDP checksum is computed go through the gathered
//      stream of the seg path (seg_tile over [ip, ip + hl + udp_len)), the
//      lanes it can't take redone by lane_payload_exact; IPv4 headers longer
//      than 40 bytes take a per-lane path of their own (tx_parse_slow);
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

// The parse on the five chunks of rx_load: header fields, ip_cksum(ip, hl)
// for 20 <= hl <= 40 (two 20-byte windows rotated out of the chunks, summed
// header-relative as csum_oc16 reads them) and the UDP length / checksum
// fields.  An IPv4 header longer than 40 bytes sets `slow` (tx_parse_slow).
__device__ __forceinline__ TxParse tx_parse(const u32x4 (&c)[5], uint64_t fa, uint32_t flen,
                                            bool valid, bool zero_udp, bool &slow)
{
    const uint32_t sf = (uint32_t)(fa & 15u);
    // frame bytes 12..23 start in chunk 0 or 1
    const uint32_t o1 = sf + 12u;
    const bool j1 = o1 >= 16u;
    const u32x4 x1 = j1 ? c[1] : c[0], y1 = j1 ? c[2] : c[1];
    uint32_t fw[3];
    win_rot(x1, y1, y1, o1 & 15u, fw);
    const RxHdr x = rx_hdr(fw[0], fw[1], fw[2], flen);
    slow = valid && x.hdr_in && x.v4 && x.hl > 40u;
    // UDP length / checksum at frame byte 14 + hl + 4: chunk 2, 3 or 4 (20 <= hl <= 40)
    const uint32_t u = sf + 18u + x.hl;
    const uint32_t ju = min(u >> 4, 4u);
    const u32x4 z4 = {0u, 0u, 0u, 0u};
    const u32x4 xu = ju <= 2u ? c[2] : (ju == 3u ? c[3] : c[4]);
    const u32x4 yu = ju <= 2u ? c[3] : (ju == 3u ? c[4] : z4);
    const uint32_t g0 = win_bytes(xu, yu, yu, u & 15u, 0);
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
        V = wsum(x.hl > 20u + 4u * m ? h1[m] : 0u, V);
    // ip->cksum: header bytes 10..11, the upper half of header dword 2
    return tx_decide(flen, valid, x, g0, fold_not(V), h0[2] >> 16, zero_udp);
}

// The same in two load rounds for this lane's frame, any IHL: the chunks
// around frame bytes 12..23 first, then, with the IHL known, the UDP fields
// and the IPv4 header's chunks (word sum at even addresses; an odd start
// folds rotl32(V, 8), the seg path's residue identity).
__device__ __forceinline__ TxParse tx_parse_slow(uint64_t fa, uint32_t flen, bool valid,
                                                 bool zero_udp, uint64_t zero)
{
    const uint64_t fend = fa + flen;
    const uint64_t a1 = fa + 12u;
    const Win2 w1 = win2_load(a1, fend, valid && flen > 12u, zero);
    uint32_t fw[3]; // frame 12..15, 16..19 = ip 2..5, 20..23 = ip 6..9
    win_rot(w1.x, w1.y, w1.y, (uint32_t)(a1 & 15u), fw);
    const RxHdr x = rx_hdr(fw[0], fw[1], fw[2], flen);
    const uint64_t ip = fa + 14u;
    const uint32_t hl = x.hl;
    const uint64_t a2 = ip + hl + 4u;
    const Win2 w2 = win2_load(a2, fend, valid && x.udp_in, zero);
    const bool hsum = valid && x.hdr_in && x.v4;
    const uint32_t sip = (uint32_t)(ip & 15u);
    const uint64_t cip = ip & ~15ull;
    const uint32_t nh = hsum ? (sip + hl + 15u) >> 4 : 0u;
    u32x4 hc[kHdrChunks];
#pragma unroll
    for (int k = 0; k < kHdrChunks; ++k)
        hc[k] = load_chunk<false>((uint32_t)k < nh ? cip + 16ull * k : zero);
    uint32_t V = 0;
#pragma unroll
    for (int k = 0; k < kHdrChunks; ++k)
        V += seg_range(hc[k], 16 * k - (int)sip, 0, (int)hl);
    const uint32_t ipck = fold_not((ip & 1u) ? __builtin_amdgcn_alignbit(V, V, 24) : V);
    const uint32_t f_ip = win_bytes(hc[0], hc[1], hc[2], sip, 2) >> 16; // header bytes 10..11
    const uint32_t g0 = win_bytes(w2.x, w2.y, w2.y, (uint32_t)(a2 & 15u), 0);
    return tx_decide(flen, valid, x, g0, ipck, f_ip, zero_udp);
}

typedef uint16_t __attribute__((address_space(1))) *gu16_ptr;
typedef uint8_t __attribute__((address_space(1))) *gu8_ptr;

// A native uint16 stored raw at any address parity, as the reference's
// `ip->cksum = ...` / `udp->cksum = ...` leave it in memory.
__device__ __forceinline__ void store_raw16(uint64_t a, uint32_t v)
{
    if (a & 1u) {
        gu8_ptr p = (gu8_ptr)(uintptr_t)a;
        p[0] = (uint8_t)v;
        p[1] = (uint8_t)(v >> 8);
    } else {
        *(gu16_ptr)(uintptr_t)a = (uint16_t)v;
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
    constexpr int UNS = 4;
    using Src = GathSrc<UNS, NT, false>;
    struct Lds {
        FlatLds<UNS> f; // slot table, row marks, prefix sums
        u32x4 stage[64 * UNS];
        u32x4 pm[17]; // seg_head's masks
    };
    __shared__ Lds L;

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
        uint32_t r = 0; // payload_cksum(ip, plen) of the bytes as loaded (need)
        const bool need = h.need && !slow;
        if (__ballot(need)) {
            const FlatTile t = flat_tile_setup<UNS, 1>(L.f, lane, ip, h.plen, h.plen, need, 0u);
            bool done = true;
            uint16_t rh = 0;
            r = seg_tile<UNS, WC_KIND_PAYLOAD, NT, false, Src, true>(
                L.f.pre, L.stage, L.pm, lane, ip, 16ull * t.cp + (ip & 15u), h.plen, need,
                t.total, Src{&L.f, t}, zero, done, rh);
            if (need && !done) // a possible wrap of the odd-start residue
                r = lane_payload_exact<NT>(ip, h.plen);
            wave_order(); // the tables are rewritten by the next tile
        }
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
    const uint64_t tiles = (n + 63) / 64;
    const int grid = (int)std::min<uint64_t>(kMaxGridBlocks, std::max<uint64_t>(1, tiles));
    const uint32_t zu = (flags & kTxZeroUdp) ? 1u : 0u;
    const bool store = !(flags & kTxNoStore);
    if (nt)
        return store ? launch_tx_one<true, true>(base, offs, flens, n, zu, status, out_ip, out_udp,
                                                 errors, grid, st)
                     : launch_tx_one<true, false>(base, offs, flens, n, zu, status, out_ip,
                                                  out_udp, errors, grid, st);
    return store ? launch_tx_one<false, true>(base, offs, flens, n, zu, status, out_ip, out_udp,
                                              errors, grid, st)
                 : launch_tx_one<false, false>(base, offs, flens, n, zu, status, out_ip, out_udp,
                                               errors, grid, st);
}

} // namespace wc
