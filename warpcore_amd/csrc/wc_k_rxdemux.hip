// wc_k_rxdemux.hip -- wc_rx_demux on gfx950: the socket every delivered frame
// belongs to (udp_rx's two w_get_sock calls, udp.c:141-156) and the delivered
// frames' indices grouped by socket, each group in ring order (DESIGN.md
// section 8, row 7).
//
// Three launches on the caller's stream, in wc_k_rxsel.hip's style: their
// order on the stream is the only ordering between the phases, no workgroup
// waits for another, no global atomic, and the output does not depend on how
// the workgroups are scheduled:
//   1. k_rxdemux_key      one lane per frame: its 16-byte record (coalesced);
//                         where af != 0 the aligned 16-byte chunks that
//                         overlap the two addresses (8 bytes at 14 + 12 for
//                         IPv4: up to two chunks; 32 bytes at 14 + 8 for
//                         IPv6: up to three), the probe of the table's LDS
//                         copy, sock[i]; and block b's count of every class
//                         into counts[class][b] (class-major);
//   2. k_rxdemux_scan     ONE workgroup: the exclusive scan of the
//                         (ns + 1) x nblocks counts in place -- class-major,
//                         so a scanned count is already the block's first
//                         position in the list -- and the 256 start entries;
//   3. k_rxdemux_scatter  block b reads its sock bytes again, ranks them the
//                         same way, puts the indices class by class into LDS
//                         and writes each class's run as one contiguous store.
// A block is kDmxBlock = 4096 frames, wave w of its sixteen takes the 256
// frames from 256 w on, 64 at a time, so (wave, step, lane) order is ring
// order; the key kernel has a wave's four steps' loads in flight together.
// A lane's rank among the lanes of its class in one step comes from ballots
// over the 8 id bits; the classes' running counts are per wave in LDS,
// added to by one lane per class and step -- nothing is ordered by an atomic.
// Classes: socket ids 0 .. ns - 1, then "unbound" (id 0xFF, row ns); id 0xFE
// (no record) and anything else a sock byte might hold belong to none.
#include "wc_rx_demux.h"

namespace wc {
namespace {

constexpr int kDmxScan = 1024;                                // threads of the scan workgroup
constexpr int kDmxScanPer = 4;                                // counts per thread and iteration
// (the block geometry, class_peers / class_rank and frame_sock are
// wc_rx_demux.h's: the RX drain kernels, wc_k_rxdrain.hip, run them too.)

// LDS of the key kernel (all dynamic, 16-byte aligned): the waves' class
// counters, then the table's slots.
constexpr uint32_t kDmxRunWords = kDmxWaves * 256u;

__global__ void __launch_bounds__(kDmxThreads)
k_rxdemux_key(const uint8_t *__restrict__ base, const uint64_t *__restrict__ offs,
              const u32x4 *__restrict__ rec, uint64_t n, const uint32_t *__restrict__ table,
              uint32_t ns, uint32_t nslots, uint8_t *__restrict__ sock,
              uint32_t *__restrict__ counts, uint32_t nblocks)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
    uint32_t *const run_all = lds, *const slots = lds + kDmxRunWords;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t k = threadIdx.x; k < kDmxRunWords; k += kDmxThreads)
        run_all[k] = 0u;
    const uint32_t tw = tab::kTabSlotWords * nslots;
    for (uint32_t k = threadIdx.x; k < tw; k += kDmxThreads)
        slots[k] = table[tab::kTabHeaderWords + k];
    __syncthreads();
    uint32_t *const run = run_all + 256u * wave;
    const uint64_t w0 = (uint64_t)blockIdx.x * kDmxBlock + (uint64_t)wave * kDmxWaveFrames;
    // the ids of the wave's steps first (their loads independent of each
    // other), then the stores and the ranking
    uint32_t ids[kDmxSteps];
#pragma unroll
    for (int step = 0; step < kDmxSteps; ++step) {
        const uint64_t i = w0 + 64u * step + lane;
        uint32_t id = kSockNone;
        if (i < n) {
            const u32x4 r = rec[i];
            if (r.z & 0xFFu) {
                id = frame_sock((uint64_t)(uintptr_t)base + offs[i], r, slots, nslots);
                id = class_counted(id, ns) ? id : kSockUnbound; // (a table of another ns)
            }
        }
        ids[step] = id;
    }
#pragma unroll
    for (int step = 0; step < kDmxSteps; ++step) {
        const uint64_t i = w0 + 64u * step + lane;
        if (i < n)
            sock[i] = (uint8_t)ids[step];
        if (counts)
            (void)class_rank(run, ids[step], ids[step] != kSockNone);
    }
    if (!counts)
        return;
    __syncthreads();
    const uint32_t c = threadIdx.x; // the first 256 threads: one id each
    if (c < 256u && class_counted(c, ns)) {
        uint32_t t = 0;
#pragma unroll
        for (int w = 0; w < kDmxWaves; ++w)
            t += run_all[256u * w + c];
        counts[(size_t)(c < ns ? c : ns) * nblocks + blockIdx.x] = t;
    }
}

// counts[0 .. (ns + 1) * nblocks) -> exclusive offsets, in place (a 64-bit
// running total: only the grand total may reach 2^32); start[s] = row s's
// first offset for s < ns, the unbound row's for ns <= s <= 254, the total
// for s = 255.
__global__ void __launch_bounds__(kDmxScan)
k_rxdemux_scan(uint32_t *__restrict__ counts, uint32_t nblocks, uint32_t ns,
               unsigned long long *__restrict__ start)
{
    __shared__ uint32_t ws[kDmxScan / 64];
    __shared__ unsigned long long unbound;
    // (<= 4096 counts of <= 4096 frames each per iteration: no wrap)
    const uint64_t carry = block_scan_counts<kDmxScan, kDmxScanPer>(
        counts, (ns + 1u) * nblocks /* <= 255 * 2^20 */, ws, [&](uint32_t i, uint64_t excl) {
            const uint32_t row = i / nblocks;
            if (i == row * nblocks) { // a row's first count
                if (row < ns)
                    start[row] = excl;
                else
                    unbound = excl;
            }
        });
    if (threadIdx.x >= ns && threadIdx.x < kDmxStarts - 1u)
        start[threadIdx.x] = unbound;
    if (threadIdx.x == kDmxStarts - 1u)
        start[threadIdx.x] = carry;
}

__global__ void __launch_bounds__(kDmxThreads)
k_rxdemux_scatter(const uint8_t *__restrict__ sock, uint64_t n, uint32_t ns,
                  const uint32_t *__restrict__ offsets, uint32_t nblocks,
                  uint32_t *__restrict__ list)
{
    __shared__ uint32_t run_all[kDmxRunWords];
    __shared__ uint32_t idx[kDmxBlock];
    __shared__ uint8_t cls[kDmxBlock];
    __shared__ uint32_t lbase[256], goff[256];
    __shared__ uint32_t ws[kDmxWaves];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t k = threadIdx.x; k < kDmxRunWords; k += kDmxThreads)
        run_all[k] = 0u;
    __syncthreads();
    uint32_t *const run = run_all + 256u * wave;
    const uint64_t w0 = (uint64_t)blockIdx.x * kDmxBlock + (uint64_t)wave * kDmxWaveFrames;
    // pass 1: the waves' class totals, as the key kernel counted them
    uint32_t ids[kDmxSteps];
#pragma unroll
    for (int step = 0; step < kDmxSteps; ++step) {
        const uint64_t i = w0 + 64u * step + lane;
        const uint32_t id = i < n ? (uint32_t)sock[i] : kSockNone;
        ids[step] = id;
        (void)class_rank(run, id, class_counted(id, ns));
    }
    __syncthreads();
    // class c's place among the block's indices in LDS (classes ascending:
    // the sockets, then 0xFF) and in the list; each wave's counters restart at
    // the first LDS position of its frames of the class
    const uint32_t c = threadIdx.x; // the first 256 threads: one id each
    const bool own = c < 256u;
    uint32_t tot = 0;
    if (own) {
        for (int w = 0; w < kDmxWaves; ++w)
            tot += run_all[256u * w + c];
    }
    uint32_t total;
    const uint32_t first = block_excl_prefix<kDmxThreads>(tot, ws, total);
    if (own) {
        uint32_t at = first;
        lbase[c] = at;
        goff[c] = class_counted(c, ns) ? offsets[(size_t)(c < ns ? c : ns) * nblocks + blockIdx.x]
                                       : 0u;
        for (int w = 0; w < kDmxWaves; ++w) {
            const uint32_t t = run_all[256u * w + c];
            run_all[256u * w + c] = at;
            at += t;
        }
    }
    __syncthreads();
    // pass 2: every counted frame's index to its place (< total <= kDmxBlock)
#pragma unroll
    for (int step = 0; step < kDmxSteps; ++step) {
        const uint32_t id = ids[step];
        const bool counted = class_counted(id, ns);
        const uint32_t p = class_rank(run, id, counted);
        if (counted && p < kDmxBlock) {
            idx[p] = (uint32_t)(w0 + 64u * step + lane);
            cls[p] = (uint8_t)id;
        }
    }
    __syncthreads();
    for (uint32_t k = threadIdx.x; k < total; k += kDmxThreads) {
        const uint32_t id = cls[k];
        const uint64_t to = (uint64_t)goff[id] + (k - lbase[id]);
        if (to < n) // (always, while sock holds what the key kernel counted)
            list[to] = idx[k];
    }
}

} // namespace

uint64_t rxdemux_scratch_bytes(uint64_t n)
{
    if (n == 0)
        return 0;
    const uint64_t nblocks = (n - 1u) / kDmxBlock + 1u;
    return 4u * (uint64_t)(tab::kTabMaxSocks + 1u) * nblocks;
}

hipError_t launch_rx_demux(const void *base, const uint64_t *offs, const void *rec, uint64_t n,
                           const void *table, uint32_t ns, uint8_t *sock, uint32_t *list,
                           uint64_t *start, void *scratch, hipStream_t st)
{
    const uint32_t nblocks = (uint32_t)((n - 1u) / kDmxBlock + 1u); // <= 2^20
    const uint32_t nslots = tab::tab_slots(ns);
    const size_t lds = 4u * (kDmxRunWords + (size_t)tab::kTabSlotWords * nslots); // <= 40 KiB
    uint32_t *counts = list ? (uint32_t *)scratch : nullptr;
    hipLaunchKernelGGL(k_rxdemux_key, dim3(nblocks), dim3(kDmxThreads), lds, st,
                       (const uint8_t *)base, offs, (const u32x4 *)rec, n, (const uint32_t *)table,
                       ns, nslots, sock, counts, nblocks);
    if (list) {
        hipLaunchKernelGGL(k_rxdemux_scan, dim3(1), dim3(kDmxScan), 0, st, counts, nblocks, ns,
                           (unsigned long long *)start);
        hipLaunchKernelGGL(k_rxdemux_scatter, dim3(nblocks), dim3(kDmxThreads), 0, st,
                           (const uint8_t *)sock, n, ns, (const uint32_t *)counts, nblocks, list);
    }
    return hipGetLastError();
}

} // namespace wc
