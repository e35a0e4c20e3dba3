// wc_k_rxneigh.hip -- the RX neighbour kernels on gfx950: what the reference
// does with the frames wc_rx_reply_plan hands to the host (WC_RR_HOST): arp_rx
// with its is-at reply, icmp6_rx's neighbour solicitation and advertisement
// branches with the advertisement icmp6_tx writes, and the (address, MAC) pair
// each of them gives neighbor_update -- decided and written on the device from
// the frame bytes and the engine table.  DESIGN.md section 4.10.  The chain,
// the record and the frame words are wc_rx_neigh.h's.
//
// k_rx_neigh_plan has k_rx_reply_plan's frame: one wave per tile of 64 frames,
// lane l = frame l, one-shot grid, XCD blocking, the next tile's metadata
// prefetched.  Per tile:
//   1. the action bytes; a tile without a HOST lane (one ballot) loads no frame
//      byte and stores 64 NONE codes;
//   2. rx_load's five chunks for the HOST lanes alone: frame bytes 0..55 hold
//      the ARP packet and, of an IPv6 frame, the EtherType, the next header and
//      the ICMPv6 type;
//   3. the engine table is read wave-uniformly (scalar loads);
//   4. a solicitation's lanes load the two chunks that hold its target, frame
//      bytes 62..77 (win2_load: each only if it overlaps the frame).
// No stream, no LDS, no atomic; the same input gives the same output.
//
// k_rx_neigh_updates and k_rx_neigh_build: one lane per list entry -- a record
// is 24 bytes, a reply 42 or 86 fixed bytes, and there is no data to copy.  A
// lane reads *count and its list entries itself, the entry one step ahead and
// what it names beside the loads of the entry in hand (the RX reply build's
// way), and derives every bound again from the frame length and the code byte
// (rn::record_of, rn::build), so a stale byte gives an empty record or length 0,
// never an access outside the frame or the slot.  Stores are plain vector
// stores: aligned dwords inside the reply, byte / 2-byte stores at its two ends
// (txb::store_words), so a neighbouring slot that shares a dword keeps every
// byte of its own.  The advertisement's checksum is formed in registers; its 37
// words cannot wrap a uint32.  The only atomic is the built count's, one per
// workgroup with a built reply.
// Roofline: latency -- a few dependent loads per frame, a few cache lines each.
#include "wc_rx_build.h"

namespace wc {
namespace {

constexpr int kRnSpan = 15; // XCD super-blocks of 2^15 tiles, as the reply plan's

// One-wave workgroups, as k_rx_reply_plan.
__global__ void __launch_bounds__(64)
k_rx_neigh_plan(const uint8_t *__restrict__ base, const uint64_t *__restrict__ offs,
                const uint16_t *__restrict__ flens, uint64_t n,
                const uint8_t *__restrict__ action, const uint32_t *__restrict__ eng,
                uint8_t *__restrict__ nact)
{
    const int lane = threadIdx.x & 63;
    const uint64_t ntiles = (n + 63) / 64;
    const uint64_t nwaves = gridDim.x;
    uint64_t tile = xcd_block(kRnSpan << 8);
    const uint64_t zero = (uint64_t)(uintptr_t)&kZeroChunk;

    uint64_t off_n;
    uint32_t flen_n;
    meta_load(offs, flens, tile * 64 + lane, n, off_n, flen_n);

    for (; tile < ntiles; tile += nwaves) {
        const uint64_t p = tile * 64 + lane;
        const bool valid = p < n;
        const uint64_t fa = (uint64_t)base + off_n;
        const uint32_t flen = flen_n;
        meta_load(offs, flens, (tile + nwaves) * 64 + lane, n, off_n, flen_n);
        const bool host = valid && action[valid ? p : 0] == rr::kHost;
        uint32_t code = rn::kNone;
        if (__ballot(host)) {
            u32x4 c[5];
            rx_load(fa, flen, host, zero, c);
            uint32_t A[5], B[5], C[4]; // frame bytes 0..19, 20..39, 40..55
            rx_words56(c, fa, A, B, C);

            rn::Look f;
            f.action = host ? rr::kHost : rn::kNone;
            f.flen = flen;
            f.f3 = A[3], f.f4 = A[4], f.f5 = B[0];
            f.tpa = (B[4] >> 16) | (C[0] << 16); // bytes 38..41
            f.b54 = (C[3] >> 16) & 0xFFu;
            code = rn::chain_head(eng, f);
            const bool tg = code == rn::kTarget;
            if (__ballot(tg)) {
                const uint64_t ta = fa + 62u;
                const Win2 w = win2_load(ta, fa + flen, tg, zero);
                uint32_t t[4];
                win_rot(w.x, w.y, w.y, (uint32_t)(ta & 15u), t);
                const uint32_t tail = rn::chain_tail(eng, t);
                if (tg)
                    code = tail;
            }
        }
        if (valid)
            nact[p] = (uint8_t)code;
    }
}

constexpr uint32_t kNeighBlock = 256;

__global__ void __launch_bounds__(kNeighBlock)
k_rx_neigh_updates(const uint8_t *__restrict__ base, const uint64_t *__restrict__ offs,
                   const uint16_t *__restrict__ flens, uint64_t n,
                   const uint8_t *__restrict__ nact, const uint32_t *__restrict__ list,
                   const unsigned long long *__restrict__ count, uint32_t m,
                   uint32_t *__restrict__ upd)
{
    // (the bodies of both: wc_rx_build.h, shared with k_rx_answer_frames)
    rx_neigh_updates_body(base, offs, flens, n, nact, list, count, m, upd,
                          (uint64_t)blockIdx.x * kNeighBlock + threadIdx.x,
                          (uint64_t)gridDim.x * kNeighBlock);
}

__global__ void __launch_bounds__(kNeighBlock)
k_rx_neigh_build(const uint8_t *__restrict__ base, const uint64_t *__restrict__ offs,
                 const uint16_t *__restrict__ flens, uint64_t n,
                 const uint8_t *__restrict__ nact, const uint32_t *__restrict__ list,
                 const unsigned long long *__restrict__ count, const uint32_t *__restrict__ eng,
                 uint8_t *out_base, const uint64_t *__restrict__ out_off, uint32_t m,
                 uint32_t slot_bytes, uint16_t *__restrict__ out_len,
                 unsigned long long *__restrict__ built)
{
    rx_neigh_build_body<kNeighBlock / 64, true>(base, offs, flens, n, nact, list, count, eng,
                                                out_base, out_off, m, slot_bytes, out_len, built,
                                                (uint64_t)blockIdx.x * kNeighBlock + threadIdx.x,
                                                (uint64_t)gridDim.x * kNeighBlock);
}

} // namespace

hipError_t launch_rx_neigh_plan(const void *base, const uint64_t *offs, const uint16_t *flens,
                                uint64_t n, const uint8_t *action, const void *eng, uint8_t *nact,
                                hipStream_t st)
{
    hipLaunchKernelGGL(k_rx_neigh_plan, dim3(tile_grid(n)), dim3(64), 0, st, (const uint8_t *)base, offs,
                       flens, n, action, (const uint32_t *)eng, nact);
    return hipGetLastError();
}

hipError_t launch_rx_neigh_updates(const void *base, const uint64_t *offs, const uint16_t *flens,
                                   uint64_t n, const uint8_t *nact, const uint32_t *list,
                                   const uint64_t *count, uint32_t m, void *upd, int cus,
                                   hipStream_t st)
{
    const int grid = list_grid<k_rx_neigh_updates, kNeighBlock, kNeighBlock>(m, cus);
    hipLaunchKernelGGL(k_rx_neigh_updates, dim3(grid), dim3(kNeighBlock), 0, st,
                       (const uint8_t *)base, offs, flens, n, nact, list,
                       (const unsigned long long *)count, m, (uint32_t *)upd);
    return hipGetLastError();
}

hipError_t launch_rx_neigh_build(const void *base, const uint64_t *offs, const uint16_t *flens,
                                 uint64_t n, const uint8_t *nact, const uint32_t *list,
                                 const uint64_t *count, const void *eng, void *out_base,
                                 const uint64_t *out_off, uint32_t m, uint32_t slot_bytes,
                                 uint16_t *out_len, uint64_t *built, int cus, hipStream_t st)
{
    const int grid = list_grid<k_rx_neigh_build, kNeighBlock, kNeighBlock>(m, cus);
    hipLaunchKernelGGL(k_rx_neigh_build, dim3(grid), dim3(kNeighBlock), 0, st,
                       (const uint8_t *)base, offs, flens, n, nact, list,
                       (const unsigned long long *)count, (const uint32_t *)eng,
                       (uint8_t *)out_base, out_off, m, slot_bytes, out_len,
                       (unsigned long long *)built);
    return hipGetLastError();
}

} // namespace wc
