// wc_k_rxdrain.hip -- wc_rx_drain on gfx950 for a ring of at most
// kRxDrainSmall frames: what wc_rx_deliver_ragged, wc_rx_demux,
// wc_rx_reply_plan and wc_rx_neigh_plan leave in their output arrays, byte for
// byte, in two launches instead of their seventeen.
// A netmap ring is 256 to 4096 slots; at that size the chain of calls costs
// its launches and nothing else.
//
// k_rx_drain_frames has the RX verdict's frame (wc_k_rx.hip): one wave per
// tile of 64 frames, lane l = frame l, one-wave workgroups, XCD blocking, the
// next tile's metadata prefetched.  Per tile, each step the statements the
// chain's own kernel runs, out of the shared headers:
//   1. rx_load's five header chunks, loaded ONCE -- every later step reads its
//      header bytes out of them;
//   2. the verdict and the delivery record (rx_parse_rec: wc_rx_hdr.h), the
//      frames whose UDP checksum must be verified through the gathered stream
//      (frame_payload_cksum), headers outside the five chunks by the two-round
//      parse (rx_parse_slow_rec);
//   3. the socket id of a frame with a record (addr_sock: wc_rx_demux.h), both
//      addresses out of the chunks (rx_words56), the table probed where it
//      lies in global memory -- at most 24.6 KiB, and a tile reads the few
//      slots its frames hash to, not a copy of all of it;
//   4. the reply chain (rr::chain_head, the ICMP / ICMPv6 sums as
//      k_rx_reply_plan takes them, rr::chain_tail: wc_rx_reply.h);
//   5. the neighbour chain (rn::chain_head, a solicitation's target bytes
//      62..77 by win2_load, rn::chain_tail: wc_rx_neigh.h);
//   6. the six per-frame arrays, each stored once.
// Every load stays inside its frame (aligned chunks that overlap it).  The
// only atomic is the drop count's, one per wave with a drop, as k_rx_verdict
// adds it.
//
// k_rx_drain_lists is ONE workgroup of 1024 threads behind it -- stream order
// is the only ordering between the two --, which reads the sock, action and
// nact bytes of the n <= 4096 frames back and writes
//   * list / start by the class ranking of k_rxdemux_key / _scatter
//     (class_peers, class_rank, per-wave running counts in LDS: wave w takes
//     the frames from 256 w on, 64 at a time, so (wave, step, lane) order is
//     ring order), all 256 start entries;
//   * rlist, nrlist and ulist with their counts: three stable compactions in
//     ring order (one ballot per step and mask, the sixteen waves' totals
//     through LDS) over WC_RR_MASK_REPLY of the action bytes and
//     WC_RN_MASK_REPLY / WC_RN_MASK_UPDATE of the nact bytes.
// List entries at and past a count are not written.  n = 0 writes the zero
// counts and starts and reads nothing.  LDS: 16 KiB of counters and a few
// hundred bytes.
//
// Neither kernel waits for another workgroup, spins, or orders anything by an
// atomic; every loop is bounded by n or by a table size; all stores are plain
// vector stores; the same input gives the same output.
// Roofline: latency -- two launches, a few dependent load rounds per tile.
#include "wc_rx_hdr.h"
#include "wc_rx_demux.h"
#include "wc_rx_neigh.h"

namespace wc {
namespace {

constexpr int kRdSpan = 15; // XCD super-blocks of 2^15 tiles, as the RX verdict's

// One-wave workgroups, as k_rx_verdict; no occupancy target (a small ring is
// bound by latency), so no register cap and no scratch.
template <bool NT>
__global__ void __launch_bounds__(64)
k_rx_drain_frames(const uint8_t *__restrict__ base, const uint64_t *__restrict__ offs,
                  const uint16_t *__restrict__ flens, uint64_t n,
                  const uint32_t *__restrict__ table, uint32_t ns, uint32_t nslots,
                  const uint32_t *__restrict__ eng, uint32_t slot_bytes,
                  uint8_t *__restrict__ verdict, u32x4 *__restrict__ rec,
                  unsigned long long *__restrict__ drops, uint8_t *__restrict__ sock,
                  uint8_t *__restrict__ action, uint16_t *__restrict__ reply_len,
                  uint8_t *__restrict__ nact)
{
    __shared__ FrameLds L;
    using Src = GathSrc<kFrameUns, NT, false>;

    const int lane = threadIdx.x & 63;
    seg_init_masks(L.pm, lane); // read after the first row group's wave_order
    const uint64_t ntiles = (n + 63) / 64;
    const uint64_t nwaves = gridDim.x;
    uint64_t tile = xcd_block(kRdSpan << 8);
    uint32_t ndrop = 0;
    const uint64_t zero = (uint64_t)(uintptr_t)&kZeroChunk;
    const uint32_t mtu = rr::eng_mtu(eng);
    const uint32_t *const slots = table + tab::kTabHeaderWords;

    uint64_t off_n;
    uint32_t flen_n;
    meta_load(offs, flens, tile * 64 + lane, n, off_n, flen_n);

    for (; tile < ntiles; tile += nwaves) {
        const uint64_t p = tile * 64 + lane;
        const bool valid = p < n;
        const uint64_t fa = (uint64_t)base + off_n;
        const uint32_t flen = flen_n;
        meta_load(offs, flens, (tile + nwaves) * 64 + lane, n, off_n, flen_n);
        const uint64_t ip = fa + 14u;

        u32x4 c[5];
        rx_load(fa, flen, valid, zero, c);

        // --- the verdict and the record (k_rx_verdict, EARLY and DELIVER) ---
        bool slow = false;
        u32x4 r4;
        const RxParse h = rx_parse_rec(c, fa, flen, valid, slow, r4);
        uint32_t v = h.verdict;
        {
            const bool need = h.need && !slow;
            const uint32_t s = frame_payload_cksum<NT>(L, lane, ip, h.plen, need, zero);
            if (need)
                v = s != 0 ? kRxBadUdpCksum : kRxOk; // udp.c:134-139
        }
        if (__ballot(slow)) { // IPv4 headers with more than 20 B of options, IHL < 5
            u32x4 rs;
            const RxParse hs = rx_parse_slow_rec(fa, flen, slow, zero, rs);
            if (slow) {
                r4 = rs;
                v = hs.verdict;
                if (hs.need)
                    v = lane_payload_exact<NT>(hs.ip, hs.plen) != 0 ? kRxBadUdpCksum : kRxOk;
            }
        }
        { // the UDP sum failed: no record after all
            const uint32_t take = v == kRxBadUdpCksum ? 0u : ~0u;
            r4 = u32x4{r4.x & take, r4.y & take, r4.z & take, r4.w & take};
        }
        ndrop += valid && rx_is_drop(v);

        // --- frame bytes 0..55 out of the same chunks: every later step ---
        uint32_t A[5], B[5], C[4]; // frame bytes 0..19, 20..39, 40..55
        rx_words56(c, fa, A, B, C);
        const RxHdr x = rx_hdr(A[3], A[4], B[0], flen);
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

        // --- the socket (k_rxdemux_key): a record's af says which addresses ---
        uint32_t sk = kSockNone;
        if (valid && (r4.z & 0xFFu)) {
            sk = addr_sock(r4, src, dst, slots, nslots);
            sk = class_counted(sk, ns) ? sk : kSockUnbound; // (a table of another ns)
        }

        // --- the reply chain (k_rx_reply_plan, d_sock given) ---
        rr::Frame f;
        f.verdict = valid ? v : 0xFFu; // (past the batch: NONE, no sum, no store)
        f.flen = flen;
        f.unbound = sk == rr::kSockUnbound;
        f.v4 = x.v4;
        f.hl = x.hl;
        f.proto = x.proto;
        f.ip_len = txb::bswap16(x.v4 ? A[4] : A[4] >> 16); // bytes 16..17 / 18..19
        f.mac_ok = rr::mac_ok(eng, A[0], A[1]);
        const rr::Match am = rr::addr_match(eng, x.v4, dst, src);
        f.dst_ok = am.dst;
        f.src_ok = am.src;

        uint32_t sum_len;
        rr::Reply r = rr::chain_head(f, mtu, slot_bytes, sum_len);
        const bool need4 = r.action == rr::kSum4 && sum_len != 0u; // (no byte: 0xFFFF)
        const bool need6 = r.action == rr::kSum6;
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

        // --- the neighbour chain (k_rx_neigh_plan) ---
        const bool host = valid && r.action == rr::kHost;
        uint32_t code = rn::kNone;
        if (__ballot(host)) {
            rn::Look k;
            k.action = host ? rr::kHost : rn::kNone;
            k.flen = flen;
            k.f3 = A[3], k.f4 = A[4], k.f5 = B[0];
            k.tpa = (B[4] >> 16) | (C[0] << 16); // bytes 38..41
            k.b54 = (C[3] >> 16) & 0xFFu;
            code = rn::chain_head(eng, k);
            const bool tg = code == rn::kTarget;
            if (__ballot(tg)) {
                const uint64_t at = fa + 62u;
                const Win2 w = win2_load(at, fa + flen, tg, zero);
                uint32_t t[4];
                win_rot(w.x, w.y, w.y, (uint32_t)(at & 15u), t);
                const uint32_t tail = rn::chain_tail(eng, t);
                if (tg)
                    code = tail;
            }
        }

        if (valid) {
            verdict[p] = (uint8_t)v;
            rx_rec_store(rec, p, r4);
            sock[p] = (uint8_t)sk;
            action[p] = (uint8_t)r.action;
            reply_len[p] = (uint16_t)r.len;
            nact[p] = (uint8_t)code;
        }
    }
    if (drops) {
        ndrop = group_sum<64>(ndrop);
        if (lane == 0 && ndrop)
            atomicAdd(drops, (unsigned long long)ndrop);
    }
}

constexpr uint32_t kRdRunWords = kDmxWaves * 256u; // the waves' class counters
constexpr int kRdMasks = 3;                        // rlist, nrlist, ulist

__device__ __forceinline__ bool mask_has(uint32_t mask, uint32_t code)
{
    return code < 32u && ((mask >> code) & 1u); // wc_rx_select's rule
}

__global__ void __launch_bounds__(kDmxThreads)
k_rx_drain_lists(const uint8_t *__restrict__ sock, const uint8_t *__restrict__ action,
                 const uint8_t *__restrict__ nact, uint32_t n, uint32_t ns,
                 uint32_t *__restrict__ list, unsigned long long *__restrict__ start,
                 uint32_t *__restrict__ rlist, unsigned long long *__restrict__ rcount,
                 uint32_t *__restrict__ nrlist, unsigned long long *__restrict__ nrcount,
                 uint32_t *__restrict__ ulist, unsigned long long *__restrict__ ucount)
{
    __shared__ uint32_t run_all[kRdRunWords];
    __shared__ uint32_t ws[kDmxWaves];
    __shared__ uint32_t wt[kRdMasks][kDmxWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t k = threadIdx.x; k < kRdRunWords; k += kDmxThreads)
        run_all[k] = 0u;
    __syncthreads();
    uint32_t *const run = run_all + 256u * wave;
    const uint32_t w0 = (uint32_t)wave * kDmxWaveFrames;
    const uint32_t masks[kRdMasks] = {rr::kMaskReply, rn::kMaskReply, rn::kMaskUpdate};
    // pass 1: the wave's class totals, and every match's rank among the wave's
    // matches of its mask (kNoRank: no match)
    constexpr uint32_t kNoRank = ~0u;
    uint32_t ids[kDmxSteps], rank[kRdMasks][kDmxSteps];
    uint32_t cnt[kRdMasks] = {0u, 0u, 0u}; // wave-uniform
#pragma unroll
    for (int step = 0; step < kDmxSteps; ++step) {
        const uint32_t i = w0 + 64u * step + lane;
        const bool in = i < n;
        const uint32_t id = in ? (uint32_t)sock[i] : kSockNone;
        const uint32_t a = in ? (uint32_t)action[i] : 0u, na = in ? (uint32_t)nact[i] : 0u;
        ids[step] = id;
        (void)class_rank(run, id, class_counted(id, ns));
#pragma unroll
        for (int m = 0; m < kRdMasks; ++m) {
            const bool hit = in && mask_has(masks[m], m == 0 ? a : na);
            const uint64_t b = __ballot(hit);
            rank[m][step] = hit ? cnt[m] + mbcnt64(b) : kNoRank;
            cnt[m] += (uint32_t)__builtin_popcountll(b);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int m = 0; m < kRdMasks; ++m)
            wt[m][wave] = cnt[m];
    }
    __syncthreads();
    // class c's place in the list (classes ascending: the sockets, then 0xFF;
    // a class that is not counted holds nothing); each wave's counters restart
    // at the list position of its first frame of the class
    const uint32_t c = threadIdx.x; // the first 256 threads: one id each
    const bool own = c < kDmxStarts;
    uint32_t tot = 0;
    if (own) {
        for (int w = 0; w < kDmxWaves; ++w)
            tot += run_all[256u * w + c];
    }
    uint32_t total;
    const uint32_t first = block_excl_prefix<kDmxThreads>(tot, ws, total);
    if (own) {
        uint32_t at = first;
        for (int w = 0; w < kDmxWaves; ++w) {
            const uint32_t t = run_all[256u * w + c];
            run_all[256u * w + c] = at;
            at += t;
        }
        // start[s]: socket s's run for s < ns, the unbound run's start for
        // ns <= s <= 254 (nothing is counted in between), the total for 255
        start[c] = c == kDmxStarts - 1u ? total : first;
    }
    __syncthreads();
    // pass 2: every counted frame's index to its place (< total <= n)
#pragma unroll
    for (int step = 0; step < kDmxSteps; ++step) {
        const uint32_t id = ids[step];
        const bool counted = class_counted(id, ns);
        const uint32_t at = class_rank(run, id, counted);
        if (counted && at < n)
            list[at] = w0 + 64u * step + lane;
    }
    // the three compactions: the matches of the waves before this one first
    uint32_t *const out[kRdMasks] = {rlist, nrlist, ulist};
    unsigned long long *const count[kRdMasks] = {rcount, nrcount, ucount};
#pragma unroll
    for (int m = 0; m < kRdMasks; ++m) {
        uint32_t before = 0, all = 0;
#pragma unroll
        for (int w = 0; w < kDmxWaves; ++w) {
            const uint32_t t = wt[m][w];
            before += w < wave ? t : 0u;
            all += t;
        }
#pragma unroll
        for (int step = 0; step < kDmxSteps; ++step) {
            const uint32_t at = before + rank[m][step];
            if (rank[m][step] != kNoRank && at < n)
                out[m][at] = w0 + 64u * step + lane;
        }
        if (threadIdx.x == 0)
            *count[m] = all;
    }
}

} // namespace

hipError_t launch_rx_drain(const void *base, const uint64_t *offs, const uint16_t *flens,
                           uint64_t n, const void *table, uint32_t ns, const void *eng,
                           uint32_t slot_bytes, const RxDrainArrays &o, bool nt, hipStream_t st)
{
    static_assert(kRxDrainSmall == kDmxBlock, "one list workgroup's reach");
    if (n > kRxDrainSmall)
        return hipErrorInvalidValue;
    if (n != 0) {
        const uint32_t nslots = tab::tab_slots(ns);
        const int grid = tile_grid(n);
#define WC_RD(N)                                                               \
    hipLaunchKernelGGL((k_rx_drain_frames<N>), dim3(grid), dim3(64), 0, st,                      \
                       (const uint8_t *)base, offs, flens, n, (const uint32_t *)table, ns, nslots, \
                       (const uint32_t *)eng, slot_bytes, o.verdict, (u32x4 *)o.rec,               \
                       (unsigned long long *)o.drops, o.sock, o.action, o.reply_len, o.nact)
        if (nt)
            WC_RD(true);
        else
            WC_RD(false);
#undef WC_RD
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    hipLaunchKernelGGL(k_rx_drain_lists, dim3(1), dim3(kDmxThreads), 0, st,
                       (const uint8_t *)o.sock, (const uint8_t *)o.action, (const uint8_t *)o.nact,
                       (uint32_t)n, ns, o.list, (unsigned long long *)o.start, o.rlist,
                       (unsigned long long *)o.rcount, o.nrlist, (unsigned long long *)o.nrcount,
                       o.ulist, (unsigned long long *)o.ucount);
    return hipGetLastError();
}

} // namespace wc
