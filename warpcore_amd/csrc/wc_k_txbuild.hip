// wc_k_txbuild.hip -- the TX build kernel on gfx950: for every frame of a
// batch, the Ethernet, IP and UDP headers the reference's udp_tx writes per
// iov (udp.c:189-220 with mk_ip4_hdr / mk_ip6_hdr and mk_eth_hdr), synthesised
// on the device from a socket table, a destination table and an 8-byte
// descriptor, both checksums included, and stored in front of the payload
// that already lies in the frame.  The header layout,
// the check chain and the stores are wc_tx_build.h's; the frame of the kernel
// (one wave per tile of 64 frames, lane l = frame l, one-shot grid, XCD
// blocking, the next tile's offsets and descriptors prefetched) and the
// gathered stream are the TX seal's (wc_k_tx.hip, wc_rx_hdr.h).
//
// Per tile:
//   1. each lane gathers its socket entry (13 dwords) and, where the
//      descriptor's dst index lies inside the table, its destination entry (6
//      dwords) -- both issued at once, the destination's used only by an
//      unconnected socket; at most 13 KB + the destinations, hot in L2.  (Not
//      staged in LDS: 13 KB beside the stream's 7984 B per one-wave workgroup
//      would leave 7 of the 16 waves a CU holds at 4 per SIMD.)  The entry
//      fixes hl, the status and the payload range; no frame byte is parsed.
//   2. the payloads [frame + 14 + hl + 8, + data_len) of the SEALED frames go
//      through the gathered stream as plain ip_cksum sums (seg_tile,
//      WC_KIND_IP): every lane gets fold(S_payload) exactly -- the stream's
//      IP kind has no lane it cannot take, so there is no per-lane redo here.
//      data_len = 0 and WC_TX_ZERO_UDP_CKSUM stream nothing.
//   3. the two checksums from registers: ip_cksum of the ten IPv4 header
//      words, and fold_not(S_pseudo + S_udphdr + fold(S_payload)).
//   4. with every load of the tile back (s_waitcnt vmcnt(0)), plain vector
//      stores of the 42 or 62 header bytes (txb::store_headers, through
//      wc_device.h's GlobalMem).
//
// No 32-bit sum wraps.  The stream's running sum may (64 jumbo payloads), but
// a payload's own sum -- at most 32747 words below 2^16 -- is the difference
// of two running sums mod 2^32, exact below 2^31.  The header sums: see
// txb::headers.  An odd payload address folds rotl32(V, 8), the seg path's
// residue identity (wc_seg.h).
//
// Stores and neighbours (store_raw16's argument in wc_k_tx.hip carries over):
// a frame's header bytes are written only by its own lane, aligned dwords
// inside [frame, frame + 14 + hl + 8) and byte / 2-byte stores at the two
// ends, so a neighbour that shares a dword, a 16-byte chunk or a cache line
// keeps every byte of its own.  The first payload chunk a lane streams may
// hold its own or a neighbour's header bytes while another wave writes them:
// they are masked out of the one register copy the chunk is used from
// (seg_head), so what they hold changes nothing.  No payload byte is written,
// and no byte outside [frame, frame + frame_len) is read or written (reads
// are the aligned 16-byte chunks that overlap the payload).
// Roofline: HBM, the payload bytes once.
#include "wc_rx_hdr.h"
#include "wc_tx_build.h"
#include "wc_tx_pump.h"

namespace wc {
namespace {

// Frame p's offset and descriptor, or frame 0's past the batch end -- with
// unconditional loads (meta_load's shape).
__device__ __forceinline__ void txb_meta_load(const uint64_t *__restrict__ offs,
                                              const uint2 *__restrict__ desc, uint64_t p,
                                              uint64_t n, uint64_t &off, uint2 &d)
{
    const uint64_t pc = p < n ? p : 0;
    off = offs[pc];
    d = desc[pc];
}

constexpr int kTxbSpan = 15; // XCD super-blocks of 2^15 tiles, as the seal's

// The body of both build kernels.  STORE = false (WC_TX_NO_STORE): the frames
// are only read.  GATED (the TX pump's build): one more
// per-frame byte, hold[p], and tp::gate in the place of the ungated kernel's
// three lines -- `built` additionally requires WC_TH_READY, so no payload byte
// of another frame is streamed and no header byte of it stored.
template <bool NT, bool STORE, bool GATED>
__device__ __forceinline__ void
tx_build_body(FrameLds &L, uint8_t *base, const uint64_t *__restrict__ offs,
              const uint2 *__restrict__ desc, uint64_t n, const uint32_t *__restrict__ socks,
              uint32_t ns, const uint32_t *__restrict__ dsts, uint32_t ndst, uint32_t slot_bytes,
              uint32_t zero_udp_flag, const uint8_t *__restrict__ hold,
              uint16_t *__restrict__ frame_len, uint8_t *__restrict__ status,
              uint16_t *__restrict__ out_ip, uint16_t *__restrict__ out_udp,
              unsigned long long *__restrict__ errors)
{
    using Src = GathSrc<kFrameUns, NT, false>;

    const int lane = threadIdx.x & 63;
    const bool zero_udp = zero_udp_flag != 0u; // wave-uniform
    seg_init_masks(L.pm, lane); // read after the first row group's wave_order
    const uint64_t ntiles = (n + 63) / 64;
    const uint64_t nwaves = gridDim.x;
    uint64_t tile = xcd_block(kTxbSpan << 8);
    uint32_t nerr = 0;
    const uint64_t zero = (uint64_t)(uintptr_t)&kZeroChunk;

    uint64_t off_n;
    uint2 desc_n;
    txb_meta_load(offs, desc, tile * 64 + lane, n, off_n, desc_n);

    for (; tile < ntiles; tile += nwaves) {
        const uint64_t p = tile * 64 + lane;
        const bool valid = p < n;
        const uint64_t fa = (uint64_t)(uintptr_t)base + off_n;
        const txb::Desc d = txb::desc_of(desc_n.x, desc_n.y);
        txb_meta_load(offs, desc, (tile + nwaves) * 64 + lane, n, off_n, desc_n);
        uint32_t hold_p = 0u;
        if constexpr (GATED)
            hold_p = hold[valid ? p : 0];

        // The table entries, only where the index lies inside the table.
        const bool sock_in = valid && d.sock < ns, dst_in = valid && d.dst < ndst;
        uint32_t w[txb::kSockWords] = {}, t[txb::kDstWords] = {};
        if (sock_in) {
            const uint32_t *e = socks + txb::kSockWords * d.sock;
#pragma unroll
            for (uint32_t k = 0; k < txb::kSockWords; ++k)
                w[k] = e[k];
        }
        if (dst_in) {
            const uint32_t *e = dsts + txb::kDstWords * d.dst;
#pragma unroll
            for (uint32_t k = 0; k < txb::kDstWords; ++k)
                t[k] = e[k];
        }
        const txb::Decide x = txb::decide(sock_in, w[0], dst_in, d.data_len, slot_bytes, zero_udp);
        tp::Gate g{x.status, x.flen, x.status <= txb::kSealedZeroUdp, false};
        if constexpr (GATED)
            g = tp::gate(hold_p, x);
        const bool built = valid && g.built;
        const bool need = built && !zero_udp && d.data_len != 0u;

        // ~ip_cksum(payload, data_len) of the lanes with `need`
        uint32_t pay = 0;
        if (__ballot(need)) {
            const uint64_t pa = fa + x.hb;
            const uint32_t len = need ? d.data_len : 0u;
            const FlatTile ft = flat_tile_setup<kFrameUns, 1>(L.f, lane, pa, len, len, need, 0u);
            bool done = true;
            uint16_t rh = 0;
            const uint32_t r = seg_tile<kFrameUns, WC_KIND_IP, NT, false, Src, false>(
                L.f.pre, L.stage, L.pm, lane, pa, 16ull * ft.cp + (pa & 15u), len, need, ft.total,
                Src{&L.f, ft}, zero, done, rh);
            pay = need ? ~r & 0xFFFFu : 0u;
            wave_order(); // the tables are rewritten by the next tile
        }
        const txb::Hdr h = txb::headers(x, d, w, t, pay, zero_udp, true);
        if constexpr (STORE) {
            // Every load of this tile's frames has returned before the first
            // header byte is written.
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (built)
                txb::store_headers(GlobalMem{}, fa, x.v4, h.h);
        }
        if (valid) {
            status[p] = (uint8_t)g.status;
            frame_len[p] = (uint16_t)(built ? x.flen : 0u);
            if (out_ip)
                out_ip[p] = (uint16_t)(built ? h.ip_hdr : 0u);
            if (out_udp)
                out_udp[p] = (uint16_t)(built ? h.udp : 0u);
        }
        if constexpr (GATED)
            nerr += valid && g.error;
        else
            nerr += valid && !built;
    }
    if (errors) {
        nerr = group_sum<64>(nerr);
        if (lane == 0 && nerr)
            atomicAdd(errors, (unsigned long long)nerr);
    }
}

// One-wave workgroups and 4 waves per SIMD, as k_tx_seal.
template <bool NT, bool STORE>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4)))
k_tx_build(uint8_t *base, const uint64_t *__restrict__ offs, const uint2 *__restrict__ desc,
           uint64_t n, const uint32_t *__restrict__ socks, uint32_t ns,
           const uint32_t *__restrict__ dsts, uint32_t ndst, uint32_t slot_bytes,
           uint32_t zero_udp_flag, uint16_t *__restrict__ frame_len, uint8_t *__restrict__ status,
           uint16_t *__restrict__ out_ip, uint16_t *__restrict__ out_udp,
           unsigned long long *__restrict__ errors)
{
    __shared__ FrameLds L;
    tx_build_body<NT, STORE, false>(L, base, offs, desc, n, socks, ns, dsts, ndst, slot_bytes,
                                    zero_udp_flag, nullptr, frame_len, status, out_ip, out_udp,
                                    errors);
}

template <bool NT>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4)))
k_tx_build_gated(uint8_t *base, const uint64_t *__restrict__ offs, const uint2 *__restrict__ desc,
                 uint64_t n, const uint32_t *__restrict__ socks, uint32_t ns,
                 const uint32_t *__restrict__ dsts, uint32_t ndst, uint32_t slot_bytes,
                 uint32_t zero_udp_flag, const uint8_t *__restrict__ hold,
                 uint16_t *__restrict__ frame_len, uint8_t *__restrict__ status,
                 uint16_t *__restrict__ out_ip, uint16_t *__restrict__ out_udp,
                 unsigned long long *__restrict__ errors)
{
    __shared__ FrameLds L;
    tx_build_body<NT, true, true>(L, base, offs, desc, n, socks, ns, dsts, ndst, slot_bytes,
                                  zero_udp_flag, hold, frame_len, status, out_ip, out_udp, errors);
}

} // namespace

template <bool NT, bool STORE>
static hipError_t launch_txb_one(void *base, const uint64_t *offs, const void *desc, uint64_t n,
                                 const void *socks, uint32_t ns, const void *dsts, uint32_t ndst,
                                 uint32_t slot_bytes, uint32_t zero_udp, uint16_t *frame_len,
                                 uint8_t *status, uint16_t *out_ip, uint16_t *out_udp,
                                 uint64_t *errors, int grid, hipStream_t st)
{
    hipLaunchKernelGGL((k_tx_build<NT, STORE>), dim3(grid), dim3(64), 0, st, (uint8_t *)base, offs,
                       (const uint2 *)desc, n, (const uint32_t *)socks, ns, (const uint32_t *)dsts,
                       ndst, slot_bytes, zero_udp, frame_len, status, out_ip, out_udp,
                       (unsigned long long *)errors);
    return hipGetLastError();
}

hipError_t launch_tx_build(void *base, const uint64_t *offs, const void *desc, uint64_t n,
                           const void *socks, uint32_t ns, const void *dsts, uint32_t ndst,
                           uint32_t slot_bytes, uint32_t flags, uint16_t *frame_len,
                           uint8_t *status, uint16_t *out_ip, uint16_t *out_udp, uint64_t *errors,
                           bool nt, hipStream_t st)
{
    const int grid = tile_grid(n);
    const uint32_t zu = (flags & kTxZeroUdp) ? 1u : 0u;
    const bool store = !(flags & kTxNoStore);
#define WC_TXB(N, S)                                                           \
    if (nt == N && store == S)                                                 \
        return launch_txb_one<N, S>(base, offs, desc, n, socks, ns, dsts, ndst, slot_bytes, zu, \
                                    frame_len, status, out_ip, out_udp, errors, grid, st);
    WC_TXB(true, true) WC_TXB(true, false) WC_TXB(false, true) WC_TXB(false, false)
#undef WC_TXB
    return hipErrorInvalidValue; // (every combination is listed above)
}

hipError_t launch_tx_build_gated(void *base, const uint64_t *offs, const void *desc, uint64_t n,
                                 const void *socks, uint32_t ns, const void *dsts, uint32_t ndst,
                                 uint32_t slot_bytes, uint32_t flags, const uint8_t *hold,
                                 uint16_t *frame_len, uint8_t *status, uint16_t *out_ip,
                                 uint16_t *out_udp, uint64_t *errors, bool nt, hipStream_t st)
{
    const int grid = tile_grid(n);
    const uint32_t zu = (flags & kTxZeroUdp) ? 1u : 0u;
#define WC_TXG(N)                                                              \
    hipLaunchKernelGGL((k_tx_build_gated<N>), dim3(grid), dim3(64), 0, st, (uint8_t *)base, offs, \
                       (const uint2 *)desc, n, (const uint32_t *)socks, ns, (const uint32_t *)dsts, \
                       ndst, slot_bytes, zu, hold, frame_len, status, out_ip, out_udp,            \
                       (unsigned long long *)errors)
    if (nt)
        WC_TXG(true);
    else
        WC_TXG(false);
#undef WC_TXG
    return hipGetLastError();
}

} // namespace wc
