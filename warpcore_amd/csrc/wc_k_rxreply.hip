// wc_k_rxreply.hip -- the RX reply kernels on gfx950: what the reference's RX
// path does with a frame beyond delivering it (eth_rx's MAC filter, ip4_rx /
// ip6_rx's address filter, icmp4_rx / icmp6_rx's checksum verdict, the echo
// replies and the port / protocol unreachables of udp_rx and ip4_rx), decided
// and written on the device from the frame bytes and the engine table (struct
// wc_rx_engine: MAC, MTU, address list).  DESIGN.md section 4.9.  The chain,
// the reply lengths, the header bytes and the data copy are wc_rx_reply.h's;
// the frame of the plan kernel (one wave per tile of 64 frames, lane l = frame
// l, one-shot grid, XCD blocking, the next tile's metadata prefetched) and the
// gathered stream are the RX verdict's (wc_k_rx.hip, wc_rx_hdr.h).
//
// k_rx_reply_plan, per tile:
//   1. rx_load's five chunks (frame bytes 0..64 at least, each chunk loaded
//      only if it overlaps the frame) give the Ethernet destination, the
//      header view (rx_hdr: EtherType, IHL of any value, lengths, protocol /
//      next header), both IP addresses and the ICMPv6 type byte; no header sum
//      is taken -- the verdict byte of the RX verdict launch in front has
//      decided it, and the chain does not decide it again;
//   2. the engine table is read wave-uniformly (scalar loads of at most 844
//      bytes, hot in the scalar cache) for the MAC and address filters;
//   3. the ICMP messages of the lanes that need a sum go through the gathered
//      stream: [ip + hl, + icmp_len) as plain ip_cksum sums (seg_tile,
//      WC_KIND_IP: no lane it cannot take), then the ICMPv6 packets [ip, ip +
//      40 + icmp_len) as payload_cksum (frame_payload_cksum with its per-lane
//      redo).  Frames that need no sum stream nothing: a tile of UDP frames is
//      one header round and two stores per lane.
// No atomic, no wait between workgroups, the same input gives the same output.
//
// k_rx_reply_build: one wave per reply at a time (replies are a minority
// class, and an MTU echo is two 1-KiB steps of the wave), eight waves per
// workgroup.  The wave reads *count and its list entries itself (one and two
// replies ahead of the one it builds), derives every length and bound again
// (rr::reply_of: a stale action byte gives length 0, never an access outside
// the frame or the slot), then
//   1. its lanes walk the aligned 16-byte chunks that lie wholly inside the
//      reply's data region; each is assembled from the two aligned source
//      chunks that overlap it (source and destination have unrelated byte
//      phases), stored, and summed as written (rr::copy_chunk); the at most
//      eight dwords in front of and behind them go the same way one dword per
//      lane (rr::copy_dword);
//   2. the sum is reduced across the wave, and lane 0 stores the 42 or 62
//      header bytes with both checksums (rr::headers, txb::store_headers).
// Stores are plain vector stores: aligned chunks and dwords inside the reply,
// byte / 2-byte stores at the two ends of the headers and of the data, so a
// neighbouring slot that shares a dword, a 16-byte chunk or a cache line keeps
// every byte of its own (store_raw16's argument in wc_k_tx.hip carries over);
// headers and data are disjoint byte ranges, so their stores need no order.
// Reads are aligned chunks and dwords that overlap the request's copied range
// or header fields, all inside the aligned 16-byte chunks that overlap the
// frame.
//
// No 32-bit sum wraps.  The plan's streams: as the RX verdict's (wc_seg.h); an
// ICMP message's own sum is at most 32768 words below 2^16.  The build: a
// reply's data is at most 65535 bytes, so the wave's total of copy_dword's
// shares is at most 32768 * 0xFFFF < 2^31; the header sums: see rr::headers.
// The only atomic is the built count's, one per workgroup with a built reply
// (as many workgroups as the device holds at once).
// Roofline: HBM -- the ICMP bytes once in the plan, once more (L2-warm behind
// the plan) in the build, the replies written once.
#include "wc_rx_build.h"

namespace wc {
namespace {

constexpr int kRrSpan = 15; // XCD super-blocks of 2^15 tiles, as the RX verdict's

// One-wave workgroups and 4 waves per SIMD, as k_rx_verdict.
template <bool NT>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4)))
k_rx_reply_plan(const uint8_t *__restrict__ base, const uint64_t *__restrict__ offs,
                const uint16_t *__restrict__ flens, uint64_t n,
                const uint8_t *__restrict__ verdict, const uint8_t *__restrict__ sock,
                const uint32_t *__restrict__ eng, uint32_t slot_bytes,
                uint8_t *__restrict__ action, uint16_t *__restrict__ reply_len)
{
    __shared__ FrameLds L;
    using Src = GathSrc<kFrameUns, NT, false>;

    const int lane = threadIdx.x & 63;
    seg_init_masks(L.pm, lane); // read after the first row group's wave_order
    const uint64_t ntiles = (n + 63) / 64;
    const uint64_t nwaves = gridDim.x;
    uint64_t tile = xcd_block(kRrSpan << 8);
    const uint64_t zero = (uint64_t)(uintptr_t)&kZeroChunk;
    const uint32_t mtu = rr::eng_mtu(eng);

    uint64_t off_n;
    uint32_t flen_n;
    meta_load(offs, flens, tile * 64 + lane, n, off_n, flen_n);

    for (; tile < ntiles; tile += nwaves) {
        const uint64_t p = tile * 64 + lane;
        const bool valid = p < n;
        const uint64_t fa = (uint64_t)base + off_n;
        const uint32_t flen = flen_n;
        meta_load(offs, flens, (tile + nwaves) * 64 + lane, n, off_n, flen_n);
        const uint64_t pc = valid ? p : 0;
        const uint32_t vd = verdict[pc];
        const uint32_t sk = sock ? sock[pc] : 0u;

        u32x4 c[5];
        rx_load(fa, flen, valid, zero, c);
        uint32_t A[5], B[5], C[4]; // frame bytes 0..19, 20..39, 40..55
        rx_words56(c, fa, A, B, C);

        const RxHdr x = rx_hdr(A[3], A[4], B[0], flen);
        rr::Frame f;
        f.verdict = valid ? vd : 0xFFu; // (past the batch: NONE, no sum, no store)
        f.flen = flen;
        f.unbound = sock != nullptr && sk == rr::kSockUnbound;
        f.v4 = x.v4;
        f.hl = x.hl;
        f.proto = x.proto;
        f.ip_len = txb::bswap16(x.v4 ? A[4] : A[4] >> 16); // bytes 16..17 / 18..19
        // IPv4 src @26, dst @30; IPv6 src @22..37, dst @38..53
        uint32_t src[4], dst[4];
        src[0] = x.v4 ? (B[1] >> 16) | (B[2] << 16) : (B[0] >> 16) | (B[1] << 16);
        src[1] = (B[1] >> 16) | (B[2] << 16);
        src[2] = (B[2] >> 16) | (B[3] << 16);
        src[3] = (B[3] >> 16) | (B[4] << 16);
        dst[0] = x.v4 ? (B[2] >> 16) | (B[3] << 16) : (B[4] >> 16) | (C[0] << 16);
        dst[1] = (C[0] >> 16) | (C[1] << 16);
        dst[2] = (C[1] >> 16) | (C[2] << 16);
        dst[3] = (C[2] >> 16) | (C[3] << 16);
        f.mac_ok = rr::mac_ok(eng, A[0], A[1]);
        const rr::Match am = rr::addr_match(eng, x.v4, dst, src);
        f.dst_ok = am.dst;
        f.src_ok = am.src;

        uint32_t sum_len;
        rr::Reply r = rr::chain_head(f, mtu, slot_bytes, sum_len);
        const bool need4 = r.action == rr::kSum4 && sum_len != 0u; // (no byte: 0xFFFF)
        const bool need6 = r.action == rr::kSum6;
        const uint64_t ip = fa + 14u;
        // The ICMP type byte at ip + hl (inside the frame wherever a byte is
        // summed), issued ahead of the stream; ICMPv6's is frame byte 54.
        const uint64_t ta = ip + x.hl;
        const u32x4 tc = load_chunk<false>(need4 ? ta & ~15ull : zero);
        uint32_t ck = 0xFFFFu;
        if (__ballot(need4)) {
            const uint32_t len = need4 ? sum_len : 0u;
            const FlatTile ft = flat_tile_setup<kFrameUns, 1>(L.f, lane, ta, len, len, need4, 0u);
            bool done = true;
            uint16_t rh = 0;
            const uint32_t s4 = seg_tile<kFrameUns, WC_KIND_IP, NT, false, Src, false>(
                L.f.pre, L.stage, L.pm, lane, ta, 16ull * ft.cp + (ta & 15u), len, need4, ft.total,
                Src{&L.f, ft}, zero, done, rh);
            if (need4)
                ck = s4;
            wave_order(); // the tables are rewritten by the next stream
        }
        const uint32_t s6 = frame_payload_cksum<NT>(L, lane, ip, need6 ? sum_len : 0u, need6, zero);
        if (need6)
            ck = s6;
        if (r.action == rr::kSum4 || r.action == rr::kSum6) {
            const uint32_t type = r.action == rr::kSum4 ? pick_byte(tc, (int)(ta & 15u))
                                                        : (C[3] >> 16) & 0xFFu;
            r = rr::chain_tail(r.action, f, ck, type, mtu, slot_bytes);
        }
        if (valid) {
            action[p] = (uint8_t)r.action;
            reply_len[p] = (uint16_t)r.len;
        }
    }
}

// kBuildWaves waves per workgroup, one reply each at a time; the grid is capped
// at what the device holds at once (launch_rx_reply_build) and strides over m,
// so the built count costs one atomic per resident workgroup: one per four
// replies serialised a flood of 2^18 echoes at 12 ns apiece, 810 us
// (profiles/ab_rxreply_build.log).
constexpr uint32_t kBuildWaves = 8;

__global__ void __launch_bounds__(64 * kBuildWaves)
k_rx_reply_build(const uint8_t *__restrict__ base, const uint64_t *__restrict__ offs,
                 const uint16_t *__restrict__ flens, uint64_t n,
                 const uint8_t *__restrict__ action, const uint32_t *__restrict__ list,
                 const unsigned long long *__restrict__ count, const uint32_t *__restrict__ eng,
                 uint8_t *out_base, const uint64_t *__restrict__ out_off, uint32_t m,
                 uint32_t slot_bytes, const uint16_t *__restrict__ ip_id,
                 uint16_t *__restrict__ out_len, unsigned long long *__restrict__ built)
{
    // (rx_reply_build_body, wc_rx_build.h: shared with k_rx_answer_frames)
    const uint32_t w = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    rx_reply_build_body<kBuildWaves, true>(base, offs, flens, n, action, list, count, eng, out_base,
                                           out_off, m, slot_bytes, ip_id, out_len, built,
                                           (uint64_t)blockIdx.x * kBuildWaves + w,
                                           (uint64_t)gridDim.x * kBuildWaves);
}

} // namespace

hipError_t launch_rx_reply_plan(const void *base, const uint64_t *offs, const uint16_t *flens,
                                uint64_t n, const uint8_t *verdict, const uint8_t *sock,
                                const void *eng, uint32_t slot_bytes, uint8_t *action,
                                uint16_t *reply_len, bool nt, hipStream_t st)
{
    const int grid = tile_grid(n);
    if (nt)
        hipLaunchKernelGGL((k_rx_reply_plan<true>), dim3(grid), dim3(64), 0, st,
                           (const uint8_t *)base, offs, flens, n, verdict, sock,
                           (const uint32_t *)eng, slot_bytes, action, reply_len);
    else
        hipLaunchKernelGGL((k_rx_reply_plan<false>), dim3(grid), dim3(64), 0, st,
                           (const uint8_t *)base, offs, flens, n, verdict, sock,
                           (const uint32_t *)eng, slot_bytes, action, reply_len);
    return hipGetLastError();
}

hipError_t launch_rx_reply_build(const void *base, const uint64_t *offs, const uint16_t *flens,
                                 uint64_t n, const uint8_t *action, const uint32_t *list,
                                 const uint64_t *count, const void *eng, void *out_base,
                                 const uint64_t *out_off, uint32_t m, uint32_t slot_bytes,
                                 const uint16_t *ip_id, uint16_t *out_len, uint64_t *built,
                                 int cus, hipStream_t st)
{
    const int grid = list_grid<k_rx_reply_build, 64 * kBuildWaves, kBuildWaves>(m, cus);
    hipLaunchKernelGGL(k_rx_reply_build, dim3(grid), dim3(64 * kBuildWaves), 0, st, (const uint8_t *)base, offs,
                       flens, n, action, list, (const unsigned long long *)count,
                       (const uint32_t *)eng, (uint8_t *)out_base, out_off, m, slot_bytes, ip_id,
                       out_len, (unsigned long long *)built);
    return hipGetLastError();
}

} // namespace wc
