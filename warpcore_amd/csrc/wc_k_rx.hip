// wc_k_rx.hip -- the RX verdict kernel on gfx950: for every frame of a netmap
// RX ring (or any batch of Ethernet frames), the checksum and header-format
// decision the reference's RX path makes, computed on the device from the
// frame bytes alone.
//
// Reference decisions restated (read, not copied):
//   eth_rx  /root/reference/lib/src/eth.c:75-86     EtherType dispatch
//   ip4_rx  /root/reference/lib/src/ip4.c:95-138    version, ip_cksum(ip, hl),
//                                                   fragment offset, protocol
//   ip6_rx  /root/reference/lib/src/ip6.c:91-111    version, next header
//   udp_rx  /root/reference/lib/src/udp.c:99-139    ip_plen, MIN(udp->len,
//           ip_plen), the zero-checksum skip and payload_cksum(ip, udp_len + hl)
// The codes are enum wc_rx_verdict (include/warpcore_gpu/wc_cksum.h); the CPU
// restatement is oracle_rx_verdict (oracle/wc_oracle.c).  Engine state (MAC
// and address filters, bound sockets) stays with the caller.
//
// One wave per tile of 64 frames (lane l = frame l), one-shot grid:
//   1. header fields: two aligned chunks around frame bytes 12..23 (EtherType,
//      version / IHL, lengths, fragment offset, protocol / next header);
//   2. with the IHL known: the UDP length and checksum fields, and for IPv4
//      the header's chunks -- its checksum is summed by the lane itself;
//   3. the frames whose UDP checksum must be verified go through the gathered
//      stream of the seg path (wc_seg.h, seg_tile over the tile's IP packets
//      [ip, ip + udp_len + hl) in packet order), the payload_cksum lanes it
//      can't take redone exactly by their own lane.
// Steps 1 and 2 (frame_hdr, frame_hdr_slow) and the stream of step 3 where it
// carries the checked frames only (frame_payload_cksum) are the TX seal
// kernel's too and live in wc_rx_hdr.h, as do the decision chain (rx_decide)
// and the delivery record, which the RX drain kernel runs as well; this file
// keeps the transposed header load and the stream that starts before the
// parse is done.
// Every load stays inside its frame (chunks that overlap [frame, frame +
// flen) only); whatever the reference would read past the frame is
// WC_RX_TRUNCATED.  Roofline: HBM, the checked frames' bytes once.
#include "wc_rx_hdr.h"

#ifdef WC_DIAG_STAMPS
// Timing diagnostic build only (tools/rx_stamps.py): per tile, lane 0 stores
// the 100-MHz wall clock (s_memrealtime, which hipcc keeps in program order
// with the loads and stores around it) at phase boundaries, the wave's
// hardware ids and the tile's stream length.
constexpr uint64_t kStampTiles = 1u << 16;
__device__ uint32_t g_rx_stamps[kStampTiles * 8];
#define WC_STAMP(k, v)                                                         \
    do {                                                                       \
        if (lane == 0 && tile < kStampTiles)                                   \
            g_rx_stamps[tile * 8 + (k)] = (v);                                 \
    } while (0)
#define WC_CLOCK() ((uint32_t)wall_clock64())
#else
#define WC_STAMP(k, v) ((void)0)
#define WC_CLOCK() 0u
#endif

namespace wc {
namespace {

// (enum wc_rx_verdict's codes, rx_is_drop, the decision chain rx_decide and the
// delivery record -- rx_record, rx_parse_rec, rx_parse_slow_rec -- are
// wc_rx_hdr.h's: the RX drain kernel, wc_k_rxdrain.hip, runs them too.)

// Steps 1 and 2 in ONE load round (rx_load, then frame_hdr on what it loaded:
// wc_rx_hdr.h), the lanes it can't take re-parsed by rx_parse_slow: two
// dependent load rounds per tile cost the mixed-size ring its headroom over
// payload_cksum alone.
//
// rx_load's five chunks, loaded transposed (HT): instruction i reads frames
// 16 i .. 16 i + 15, four lanes per frame, lane 4 f' + j its chunk j -- 64
// contiguous bytes per frame, one cache line instead of four separate
// 16-byte requests (five one-lane-per-frame loads put 320 line requests per
// tile in front of the stream's ~140).  Chunk 4 (frame bytes past 64 - sf)
// is loaded per lane, and only by lanes whose start phase sf > 2 may need it
// (the parse reads frame bytes < 14 + 40 + 8 = 62).  rx_hdr_gather then hands
// each lane its frame's chunks through LDS.
// Each lane finds its frame's address and length in a 1-KB LDS table the
// tile's lanes write first (one 16-byte store, four 16-byte reads, all
// issued back to back), not by twelve cross-lane shuffles, each a dependent
// LDS round trip before the next header load.  `tbl` is the tile's
// descriptor table, which flat_tile_setup rewrites afterwards.
__device__ __forceinline__ void rx_load_t(uint64_t fa, uint32_t flen, bool valid, uint64_t zero,
                                          int lane, u32x4 *tbl, u32x4 (&hx)[4], u32x4 &c4)
{
    const uint32_t lv = valid ? flen : 0u;
    tbl[lane] = u32x4{(uint32_t)fa, (uint32_t)(fa >> 32), lv, 0u};
    wave_order();
    u32x4 e[4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
        e[i] = tbl[16 * i + (lane >> 2)]; // frame 16 i + lane / 4
    wave_order(); // (the table is rewritten by flat_tile_setup)
    const uint64_t j16 = 16ull * (uint32_t)(lane & 3);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint64_t faf = (uint64_t)e[i].x | ((uint64_t)e[i].y << 32);
        const uint32_t lf = e[i].z;
        const uint64_t a = (faf & ~15ull) + j16;
        hx[i] = load_chunk<false>(lf != 0u && a < faf + lf ? a : zero);
    }
    const uint64_t a4 = (fa & ~15ull) + 64u;
    c4 = load_chunk<false>(lv != 0u && (fa & 15u) > 2u && a4 < fa + lv ? a4 : zero);
}

// The hand-off is XOR-swizzled: chunk j of frame f sits in slot
// 4 f + (j ^ ((f >> 2) & 3)).  Unswizzled (slot 4 f + j), the read of chunk k
// by lane f -- 16 B at a 64-B lane stride -- put the four lanes f, f + 4,
// f + 8, f + 12 of a ds_read_b128 lane group on the same banks (bank =
// (address / 4) mod 64): a 4-way conflict on every read, 2.85 M conflict
// cycles on the mixed-size ring against 1.28 M for the plain stream
// (profiles/pmc_r05_rx_instr.txt).  Swizzled, each 16-lane group reads 16
// distinct 16-B bank slots (its lanes are 16 distinct residues mod 16), and
// the stores stay conflict-free (each 8-lane ds_write_b128 group still
// covers 8 consecutive slots, permuted).
__device__ __forceinline__ void rx_hdr_gather(u32x4 *stage, int lane, const u32x4 (&hx)[4],
                                              const u32x4 &c4, u32x4 (&c)[5])
{
    const int ws = lane ^ ((lane >> 4) & 3); // frame 16 i + lane / 4, chunk lane % 4
#pragma unroll
    for (int i = 0; i < 4; ++i)
        stage[64 * i + ws] = hx[i];
    wave_order();
    const int rs = (lane >> 2) & 3;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        c[k] = stage[4 * lane + (k ^ rs)];
    c[4] = c4;
    wave_order(); // stage is rewritten by the stream's first row group
}

// The one-round parse (frame_hdr, wc_rx_hdr.h) and the decision on it.  `slow`:
// an IPv4 header longer than 40 bytes (options > 20 B) is not inside the five
// chunks; and for a malformed IHL < 5 ip4_rx still rules on ip_cksum(ip, hl)
// (ip4.c:111), a sum over fewer than the 20 bytes frame_hdr always takes --
// both are parsed again by rx_parse_slow.  (The TX seal rules IHL < 5
// MALFORMED before the header sum matters: tx_parse asks for hl > 40 only.)
__device__ __forceinline__ RxParse rx_parse(const u32x4 (&c)[5], uint64_t fa, uint32_t flen,
                                            bool valid, bool &slow)
{
    const FrameHdr f = frame_hdr(c, fa, flen);
    slow = valid && f.x.hdr_in && f.x.v4 && (f.x.hl > 40u || f.x.hl < 20u);
    return rx_decide(fa, flen, valid, f.x, f.g0, (uint16_t)f.ipck);
}

// The fallback of rx_parse: two load rounds, any IHL (frame_hdr_slow).
__device__ __forceinline__ RxParse rx_parse_slow(uint64_t fa, uint32_t flen, bool valid,
                                                 uint64_t zero)
{
    const FrameHdr f = frame_hdr_slow(fa, flen, valid, zero);
    return rx_decide(fa, flen, valid, f.x, f.g0, (uint16_t)f.ipck);
}

// Kernel modes (launch_rx_verdict), all giving the same verdicts:
//   EARLY  the header parse completes BEFORE the stream, which then carries
//          only the frames that need the UDP check and only their checked
//          range [ip, ip + udp_len + hl) -- one load round trip per tile
//          more; otherwise every frame with >= 28 IP bytes starts streaming
//          while the parse is in flight;
//   HT     the header chunks are loaded transposed (rx_load_t);
//   SKIP   (with !EARLY) once parsed, frames that need no check leave the
//          stream: its later row groups read the zero chunk for them.
//   TALLY  (with the default ADAPT mode, wc_cksum_api.cpp rx_launch) every
//          64th tile writes how many of its frames needed no UDP check (not
//          IP, not UDP, zero checksum, drops) and how many it held, one word
//          per tile `tally[tile / 64] = gen << 16 | ruled_out << 8 | frames`,
//          with a plain store into mapped host memory; the host picks EARLY
//          or HT for the device's next launch from the newest complete
//          tally.  No load and no atomic in the kernel: a first version kept
//          one device counter per launch that every tile read and every 8th
//          tile added to, and the same-address atomics serialised the mixed
//          ring from 113 to 458 us (profiles/ab_r05_rx_adapt.log).
// (4 waves per SIMD for every mode: capping the EARLY kernels at 96 VGPRs
// for 5 spilled 4 of them and took the mixed ring from 114 to 141 us,
// profiles/ab_r04_rx_early_waves.log.)
// One-wave workgroups: a wave's slot is handed to the next tile as soon as
// its own tile is done, not when the slowest of four is (mixed-size ring with
// ARP frames 91.8 -> 89.1 us, the others unchanged: profiles/ab_r06m_rx_waves.log).
constexpr int kRxSpan = 15; // XCD super-blocks of 2^15 tiles, as the seg kernel's

//   DELIVER (wc_rx_deliver_*; HT, no SKIP) also writes rec[p], the frame's
//          struct wc_rx_record, one 16-byte store per lane where the parse
//          has it (inside the Late hook, or right after rx_parse), so that no
//          record register lives across the stream: a real record where the
//          parse accepts the frame pending the UDP sum, zeros otherwise; the
//          few lanes whose UDP sum then fails store zeros over theirs (the
//          same lane, the same address: in program order).
// The record array is a trailing parameter PACK: empty for the plain verdict
// kernels, whose signature, name and code stay what they were before DELIVER
// (tools/kres.sh), one `u32x4 *` for the DELIVER kernels.
__device__ __forceinline__ u32x4 *rx_rec_arg() { return nullptr; }
__device__ __forceinline__ u32x4 *rx_rec_arg(u32x4 *rec) { return rec; }

template <bool NT, bool EARLY, bool HT, bool SKIP, bool TALLY, typename... Rec>
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4)))
k_rx_verdict(const uint8_t *__restrict__ base, const uint64_t *__restrict__ offs,
             const uint16_t *__restrict__ flens, uint64_t n, uint8_t *__restrict__ verdict,
             unsigned long long *__restrict__ drops, uint32_t *__restrict__ tally, uint32_t gen,
             Rec... rec_arg)
{
    constexpr bool DELIVER = sizeof...(Rec) == 1;
    static_assert(sizeof...(Rec) <= 1, "no record array, or one");
    static_assert(!DELIVER || (HT && !SKIP), "deliver launches: transposed headers, no SKIP");
    [[maybe_unused]] u32x4 *const __restrict__ rec = rx_rec_arg(rec_arg...);
    __shared__ FrameLds L;

    const int lane = threadIdx.x & 63;
    seg_init_masks(L.pm, lane); // read after the first row group's wave_order
    const uint64_t ntiles = (n + 63) / 64;
    const uint64_t nwaves = gridDim.x;
    uint64_t tile = xcd_block(kRxSpan << 8);
    uint32_t ndrop = 0;
    const uint64_t zero = (uint64_t)(uintptr_t)&kZeroChunk;

    uint64_t off_n;
    uint32_t flen_n;
    meta_load(offs, flens, tile * 64 + lane, n, off_n, flen_n);

    for (; tile < ntiles; tile += nwaves) {
        WC_STAMP(0, WC_CLOCK());
        const uint64_t p = tile * 64 + lane;
        const bool valid = p < n;
        const uint64_t fa = (uint64_t)base + off_n;
        const uint32_t flen = flen_n;
        meta_load(offs, flens, (tile + nwaves) * 64 + lane, n, off_n, flen_n);

        u32x4 c[5];
        u32x4 hx[4], c4;
        if constexpr (HT)
            rx_load_t(fa, flen, valid, zero, lane, reinterpret_cast<u32x4 *>(L.f.desc), hx, c4);
        else
            rx_load(fa, flen, valid, zero, c);
        WC_STAMP(1, WC_CLOCK());
#ifdef WC_DIAG_STAMPS
        if (lane == 0 && tile < kStampTiles) {
            g_rx_stamps[tile * 8 + 6] = __builtin_amdgcn_s_getreg(4 | (31 << 11));  // HW_ID
            g_rx_stamps[tile * 8 + 7] = __builtin_amdgcn_s_getreg(20 | (15 << 11)); // XCC_ID
        }
#endif
        auto headers = [&] { // this lane's frame chunks 0..4 (HT: through LDS)
            if constexpr (HT)
                rx_hdr_gather(L.stage, lane, hx, c4, c);
        };
        const uint64_t ip = fa + 14u;
        bool slow = false;
        RxParse h{};
        uint32_t v;
// rx_parse; DELIVER: and the record it has, stored at once.  (A macro and
// `if constexpr` around the plain kernels' own statements, not a lambda: the
// plain kernels must compile to exactly what they were.)
#define WC_RX_PARSE()                                                          \
    do {                                                                       \
        if constexpr (DELIVER) {                                               \
            u32x4 r_;                                                          \
            h = rx_parse_rec(c, fa, flen, valid, slow, r_);                    \
            if (valid)                                                         \
                rx_rec_store(rec, p, r_);                                      \
        } else {                                                               \
            h = rx_parse(c, fa, flen, valid, slow);                            \
        }                                                                      \
    } while (0)
// The UDP sum failed: no record after all.
#define WC_RX_TAKE_BACK(failed)                                                \
    do {                                                                       \
        if constexpr (DELIVER) {                                               \
            if (failed)                                                        \
                rx_rec_store(rec, p, rx_zero_record());                        \
        }                                                                      \
    } while (0)
        if constexpr (EARLY) {
            headers();
            WC_RX_PARSE();
            v = h.verdict;
            const bool need = h.need && !slow;
            const uint32_t r = frame_payload_cksum<NT>(L, lane, ip, h.plen, need, zero);
            if (need)
                v = r != 0 ? kRxBadUdpCksum : kRxOk; // udp.c:134-139
            WC_RX_TAKE_BACK(need && r != 0);
        } else {
            constexpr int UNS = kFrameUns;
            using Src = GathSrc<UNS, NT, SKIP>;
            // Header chunks first; then every frame that may need the UDP
            // check (>= 28 IP bytes) streams its IP bytes [ip, ip + room) as
            // the seg path's gathered stream, and the parse completes once
            // that stream's first row group is in flight (seg_tile's Late
            // hook): the checked range [ip, ip + udp_len + hl) is a prefix of
            // the streamed one.  A frame that turns out not to need the check
            // was read for the first row group only (SKIP).
            const uint32_t room = flen >= 14u ? flen - 14u : 0u;
            const bool spec = valid && room >= 28u;
            if (__ballot(spec)) {
                const FlatTile t = flat_tile_setup<UNS, 1>(L.f, lane, ip, room, room, spec, 0u);
                bool need = false;
                auto late = [&](uint32_t &len, bool &on) {
                    headers();
                    WC_RX_PARSE();
                    need = h.need && !slow;
                    on = need;
                    len = need ? h.plen : 0u;
                    WC_STAMP(2, WC_CLOCK());
                    if constexpr (SKIP) {
                        if (spec && !need) // its later chunks: the zero chunk
                            L.f.desc[t.rank].info = 1u << 31;
                        wave_order();
                    }
                };
                bool done = true;
                uint16_t rh = 0;
                uint16_t r = seg_tile<UNS, WC_KIND_PAYLOAD, NT, false, Src, true, decltype(late)>(
                    L.f.pre, L.stage, L.pm, lane, ip, 16ull * t.cp + (ip & 15u), room, spec,
                    t.total, Src{&L.f, t}, zero, done, rh, late);
                WC_STAMP(3, WC_CLOCK());
                WC_STAMP(5, t.total);
                if (need && !done) // header longer than the packet, or a possible wrap
                    r = lane_payload_exact<NT>(ip, h.plen);
                v = h.verdict;
                if (need)
                    v = r != 0 ? kRxBadUdpCksum : kRxOk; // udp.c:134-139
                WC_RX_TAKE_BACK(need && r != 0);
                wave_order(); // the tables are rewritten by the next tile
            } else {
                headers();
                WC_RX_PARSE();
                v = h.verdict;
            }
        }
        if constexpr (TALLY) {
            if ((tile & 63u) == 0 && (tile >> 6) < kRxTallyWords) { // a sample of the mix
                const uint32_t nv = __builtin_popcountll(__ballot(valid));
                const uint32_t nout = __builtin_popcountll(__ballot(valid && !h.need));
                if (lane == 0)
                    __hip_atomic_store(&tally[tile >> 6], (gen << 16) | (nout << 8) | nv,
                                       __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
            }
        }
        if (__ballot(slow)) { // IPv4 headers with more than 20 B of options, IHL < 5
            if constexpr (DELIVER) { // (stored before the exact sum, taken back after it)
                u32x4 r;
                const RxParse hs = rx_parse_slow_rec(fa, flen, slow, zero, r);
                if (slow) {
                    rx_rec_store(rec, p, r);
                    v = hs.verdict;
                    if (hs.need)
                        v = lane_payload_exact<NT>(hs.ip, hs.plen) != 0 ? kRxBadUdpCksum : kRxOk;
                    WC_RX_TAKE_BACK(hs.need && v == kRxBadUdpCksum);
                }
            } else {
                const RxParse hs = rx_parse_slow(fa, flen, slow, zero);
                if (slow) {
                    v = hs.verdict;
                    if (hs.need)
                        v = lane_payload_exact<NT>(hs.ip, hs.plen) != 0 ? kRxBadUdpCksum : kRxOk;
                }
            }
        }
        if (valid)
            verdict[p] = (uint8_t)v;
        ndrop += valid && rx_is_drop(v);
        WC_STAMP(4, WC_CLOCK());
    }
#undef WC_RX_PARSE
#undef WC_RX_TAKE_BACK
    if (drops) {
        ndrop = group_sum<64>(ndrop);
        if (lane == 0 && ndrop)
            atomicAdd(drops, (unsigned long long)ndrop);
    }
}

} // namespace

template <bool NT, bool EARLY, bool HT, bool SKIP, bool TALLY, bool DELIVER = false>
static hipError_t launch_rx_one(const void *base, const uint64_t *offs, const uint16_t *flens,
                                uint64_t n, uint8_t *verdict, uint64_t *drops, int grid,
                                hipStream_t st, uint32_t *tally, uint32_t gen,
                                void *rec = nullptr)
{
    if constexpr (DELIVER)
        hipLaunchKernelGGL((k_rx_verdict<NT, EARLY, HT, SKIP, TALLY, u32x4 *>), dim3(grid),
                           dim3(64), 0, st, (const uint8_t *)base, offs, flens, n, verdict,
                           (unsigned long long *)drops, tally, gen, (u32x4 *)rec);
    else
        hipLaunchKernelGGL((k_rx_verdict<NT, EARLY, HT, SKIP, TALLY>), dim3(grid), dim3(64), 0,
                           st, (const uint8_t *)base, offs, flens, n, verdict,
                           (unsigned long long *)drops, tally, gen);
    return hipGetLastError();
}

hipError_t launch_rx_verdict(const void *base, const uint64_t *offs, const uint16_t *flens,
                             uint64_t n, uint8_t *verdict, uint64_t *drops, bool nt,
                             hipStream_t st, int mode, uint32_t *tally, uint32_t gen,
                             int max_grid, void *rec)
{
    const uint64_t tiles = (n + 63) / 64;
    // One tile per wave (one-shot); max_grid > 0 (WC_RX_GRID, tools) caps the
    // grid, each wave then walks several tiles with the next tile's metadata
    // prefetched.
    const uint64_t cap = max_grid > 0 ? (uint64_t)max_grid : kMaxGridBlocks;
    const int grid = (int)std::min<uint64_t>(cap, std::max<uint64_t>(1, tiles));
    // EARLY streams only the checked frames: SKIP has nothing to skip there,
    // and is dropped so that NT and HDRT are still honoured.
    const bool early = mode & kRxEarly, ht = mode & kRxHdrT, skip = (mode & kRxSkip) && !early;
    // ADAPT: the host chose EARLY or HT; the kernel tallies
    const bool tal = tally && !skip && ht;
    if (rec) { // deliver launches: the transposed-header kernels only (HDRT / SKIP ignored)
#define WC_RXD(N, E, T)                                                        \
    if (nt == N && early == E && (tally != nullptr) == T)                      \
        return launch_rx_one<N, E, true, false, T, true>(                      \
            base, offs, flens, n, verdict, drops, grid, st, T ? tally : nullptr, T ? gen : 0u,  \
            rec);
        WC_RXD(true, false, false) WC_RXD(true, false, true) WC_RXD(true, true, false)
        WC_RXD(true, true, true) WC_RXD(false, false, false) WC_RXD(false, false, true)
        WC_RXD(false, true, false) WC_RXD(false, true, true)
#undef WC_RXD
    }
#define WC_RX(N, E, H, S, T)                                                   \
    if (nt == N && early == E && ht == H && skip == S && tal == T)             \
        return launch_rx_one<N, E, H, S, T>(base, offs, flens, n, verdict, drops, grid, st,   \
                                            T ? tally : nullptr, T ? gen : 0u);
#define WC_RX_NT(N)                                                            \
    WC_RX(N, false, false, false, false) WC_RX(N, false, false, true, false)   \
    WC_RX(N, false, true, false, false) WC_RX(N, false, true, true, false)     \
    WC_RX(N, true, false, false, false) WC_RX(N, true, true, false, false)     \
    WC_RX(N, false, true, false, true) WC_RX(N, true, true, false, true)
    WC_RX_NT(true)
    WC_RX_NT(false)
#undef WC_RX_NT
#undef WC_RX
    return hipErrorInvalidValue; // (every combination is listed above)
}

} // namespace wc

#ifdef WC_DIAG_STAMPS
extern "C" int wc_diag_rx_stamps(uint32_t *host, uint64_t words)
{
    if (words > kStampTiles * 8)
        words = kStampTiles * 8;
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_rx_stamps), words * 4, 0,
                                    hipMemcpyDeviceToHost);
}
#endif
