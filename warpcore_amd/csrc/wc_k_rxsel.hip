// wc_k_rxsel.hip -- wc_rx_select on gfx950: a stable stream compaction over
// the RX verdict bytes.  list[0 .. *count) = the frame indices i, ascending,
// whose code's bit is set in `mask`.
//
// Three launches on the caller's stream; their order on the stream is the
// only ordering between the phases -- no workgroup waits for another inside
// a kernel (no look-back, no flag), and no atomic anywhere:
//   1. k_rxsel_count    block b counts the matches among its kSelBlock
//                       16-byte chunks of verdict bytes into scratch[b];
//   2. k_rxsel_scan     ONE workgroup turns the block counts into exclusive
//                       offsets in place, kSelScan counts per iteration with
//                       a 64-bit running total, which it stores as *count;
//   3. k_rxsel_scatter  block b reads its chunks again, ranks its lanes'
//                       matches (DPP wave prefix, the four wave totals through
//                       LDS), puts the indices in rank order into LDS and
//                       writes them out as one contiguous run from
//                       list[scratch[b]] on: coalesced whatever the density.
// The verdict bytes are read as the aligned 16-byte chunks of the address
// space that overlap [verdict, verdict + n) (any alignment of `verdict`; a
// chunk that overlaps the array lies in a page the array touches), the bytes
// of the first and last chunk outside the array masked off.
// n <= 2^32: indices fit a uint32, a block's offset is below 2^32 (it counts
// matches before the block), only the total may be 2^32 -- hence 64 bits.
#include "wc_device.h"

namespace wc {
namespace {

constexpr int kSelThreads = 256;
constexpr uint32_t kSelBlock = kSelThreads; // chunks per block: 4096 verdict bytes
constexpr int kSelScan = 1024;              // block counts per scan iteration

// Bit j set: byte j of the chunk is a verdict of the array (not before its
// first or past its last byte) and its code's bit is set in mask.  `first` =
// the frame index of the chunk's byte 0 (negative in the first chunk of an
// unaligned array).
__device__ __forceinline__ uint32_t sel_match(const u32x4 &d, uint32_t mask, int64_t first,
                                              uint64_t n)
{
    uint32_t m = 0;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const uint32_t b = pick_byte(d, j);
        m |= (b < 32u ? (mask >> b) & 1u : 0u) << j;
    }
    const int64_t left = (int64_t)n - first; // bytes of the array from the chunk's byte 0 on
    const uint32_t jlo = first < 0 ? (uint32_t)(-first) : 0u;
    const uint32_t jhi = left < 16 ? (uint32_t)left : 16u;
    return m & ((1u << jhi) - 1u) & ~((1u << jlo) - 1u);
}

// This lane's chunk of block `blk`, its match bits and the index of its byte 0.
__device__ __forceinline__ uint32_t sel_lane(const uint8_t *verdict, uint64_t n, uint32_t mask,
                                             uint64_t nchunks, int64_t &first)
{
    const uint64_t addr = (uint64_t)(uintptr_t)verdict;
    const uint32_t head = (uint32_t)(addr & 15u);
    const uint64_t k = (uint64_t)blockIdx.x * kSelBlock + threadIdx.x;
    first = (int64_t)(16ull * k) - (int64_t)head;
    if (k >= nchunks)
        return 0u;
    const u32x4 d = load_chunk<false>((addr & ~15ull) + 16ull * k);
    return sel_match(d, mask, first, n);
}

__global__ void __launch_bounds__(kSelThreads)
k_rxsel_count(const uint8_t *__restrict__ verdict, uint64_t n, uint32_t mask, uint64_t nchunks,
              uint32_t *__restrict__ counts)
{
    __shared__ uint32_t ws[kSelThreads / 64];
    int64_t first;
    const uint32_t m = sel_lane(verdict, n, mask, nchunks, first);
    uint32_t total;
    (void)block_excl_prefix<kSelThreads>((uint32_t)__builtin_popcount(m), ws, total);
    if (threadIdx.x == 0)
        counts[blockIdx.x] = total;
}

// counts[0 .. nblocks) -> exclusive offsets, in place; *count = the total.
__global__ void __launch_bounds__(kSelScan)
k_rxsel_scan(uint32_t *__restrict__ counts, uint32_t nblocks, unsigned long long *__restrict__ count)
{
    __shared__ uint32_t ws[kSelScan / 64];
    // (<= 1024 blocks x 4096 matches per iteration: no wrap)
    const uint64_t carry =
        block_scan_counts<kSelScan, 1>(counts, nblocks, ws, [](uint32_t, uint64_t) {});
    if (threadIdx.x == 0)
        *count = carry;
}

__global__ void __launch_bounds__(kSelThreads)
k_rxsel_scatter(const uint8_t *__restrict__ verdict, uint64_t n, uint32_t mask, uint64_t nchunks,
                const uint32_t *__restrict__ offsets, uint32_t *__restrict__ list)
{
    __shared__ uint32_t ws[kSelThreads / 64];
    __shared__ uint32_t idx[kSelBlock * 16];
    int64_t first;
    uint32_t m = sel_lane(verdict, n, mask, nchunks, first);
    uint32_t total;
    uint32_t r = block_excl_prefix<kSelThreads>((uint32_t)__builtin_popcount(m), ws, total);
    while (m) { // r + popcount(m) <= total <= kSelBlock * 16
        idx[r++] = (uint32_t)(first + __builtin_ctz(m));
        m &= m - 1u;
    }
    __syncthreads();
    uint32_t *out = list + offsets[blockIdx.x];
    for (uint32_t k = threadIdx.x; k < total; k += kSelThreads)
        out[k] = idx[k];
}

__host__ uint64_t sel_chunks(const uint8_t *verdict, uint64_t n)
{
    return (((uint64_t)(uintptr_t)verdict & 15u) + n + 15u) / 16u;
}

} // namespace

// One count per block, for an array at the worst alignment.
uint64_t rxsel_scratch_bytes(uint64_t n)
{
    if (n == 0)
        return 0;
    const uint64_t chunks = n / 16u + 2u; // >= (15 + n + 15) / 16, without overflow
    return 4u * ((chunks + kSelBlock - 1u) / kSelBlock);
}

hipError_t launch_rx_select(const uint8_t *verdict, uint64_t n, uint32_t mask, uint32_t *list,
                            uint64_t *count, void *scratch, hipStream_t st)
{
    const uint64_t nchunks = sel_chunks(verdict, n);
    const uint32_t nblocks = (uint32_t)((nchunks + kSelBlock - 1u) / kSelBlock); // <= 2^20 + 1
    uint32_t *counts = (uint32_t *)scratch;
    hipLaunchKernelGGL(k_rxsel_count, dim3(nblocks), dim3(kSelThreads), 0, st, verdict, n, mask,
                       nchunks, counts);
    hipLaunchKernelGGL(k_rxsel_scan, dim3(1), dim3(kSelScan), 0, st, counts, nblocks,
                       (unsigned long long *)count);
    hipLaunchKernelGGL(k_rxsel_scatter, dim3(nblocks), dim3(kSelThreads), 0, st, verdict, n, mask,
                       nchunks, (const uint32_t *)counts, list);
    return hipGetLastError();
}

} // namespace wc
