// wc_k_txpump.hip -- the TX pump's plan launch on gfx950: for at most
// tp::kSmall frames, tp::kSmallDst destinations and as many solicitation slots
// (one workgroup zeroes no longer a length array), everything wc_tx_resolve,
// wc_tx_hold_plan (both with their lists) and wc_tx_solicit_build leave, byte
// for byte, from ONE workgroup of 1024 threads.  The
// gated build that follows it on the stream is wc_k_txbuild.hip's.
//
// Wave w takes the indices from 256 w on, 64 at a time, so (wave, step, lane)
// order is index order and a stable compaction is one ballot per step with the
// sixteen waves' totals passed through LDS (k_rx_drain_lists' scheme), over two
// index spaces:
//   destinations  A. tn::lookup on the table where it lies (plain loads: nobody
//                    writes it), the dmac bytes, the state byte into an LDS copy;
//                    a miss enters the de-duplication set -- in LDS, by
//                    wc_tx_neigh.h's own resolve_find lines -- with an LDS
//                    compare-and-swap and an LDS max of ~k.
//                 B. resolve_mark: a miss that is not its slot's lowest index is
//                    MISS_DUP.
//                 C. the state bytes to global memory; the MISS count per wave.
//                 D. the ascending miss list (global and an LDS copy), its count.
//                 E. solicitation j < MIN(count, m) from the LDS copy of the
//                    list, by k_tx_solicit_build's lines; the other lengths 0;
//                    the built count through one LDS counter.
//   frames        C. tn::hold_of per descriptor, d_state[dst] read from the LDS
//                    copy -- no thread of this launch loads a global byte
//                    another thread of it stored; the HELD count per wave.
//                 D. the ascending held list, its count.
// A .. E are separated by workgroup barriers; no thread waits for another
// anywhere else, nothing spins, and every loop is bounded by ndst, n, m, the
// table's cap or the set's size.  "Lowest index wins" holds whatever the
// interleaving (wc_tx_neigh.h says why).  All global stores are plain vector
// stores; there is no global atomic.  LDS: the set (64 KiB at 4096
// destinations), where and the list copy (16 KiB each), the state bytes (4 KiB)
// -- one workgroup may declare up to 160 KiB on this part.
// Roofline: latency -- a hash and a few dependent loads per thread, five
// barriers.
#include "wc_rx_hdr.h"
#include "wc_tx_pump.h"

namespace wc {
namespace {

constexpr int kTpThreads = 1024, kTpWaves = kTpThreads / 64;
constexpr uint32_t kTpReach = 4096u;           // indices one workgroup takes
constexpr uint32_t kTpWaveSpan = kTpReach / kTpWaves; // 256: four steps of 64
constexpr int kTpSteps = kTpWaveSpan / 64;
constexpr uint32_t kTpSetWords = 4u * kTpReach; // 2 set_slots(4096)
static_assert(tp::kSmall == kTpReach && tp::kSmallDst == kTpReach, "one workgroup's reach");

// wc_tx_neigh.h's Words for this launch: the tables in global memory and the
// set, where and state bytes in LDS, through generic pointers.  ld_now / cas /
// amax are only ever applied to the set's words.
struct PumpWords {
    __device__ __forceinline__ uint32_t ld(const uint32_t *p) const { return *p; }
    __device__ __forceinline__ uint32_t ld_now(const uint32_t *p) const
    {
        return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    __device__ __forceinline__ uint32_t ld8(const uint8_t *p) const { return *p; }
    __device__ __forceinline__ void st(uint32_t *p, uint32_t v) const { *p = v; }
    __device__ __forceinline__ void st16(uint32_t *p, uint32_t v) const
    {
        *reinterpret_cast<uint16_t *>(p) = (uint16_t)v;
    }
    __device__ __forceinline__ void st8(uint8_t *p, uint32_t v) const { *p = (uint8_t)v; }
    __device__ __forceinline__ uint32_t cas(uint32_t *p, uint32_t expect, uint32_t want) const
    {
        return atomicCAS(p, expect, want);
    }
    __device__ __forceinline__ void amax(uint32_t *p, uint32_t v) const { atomicMax(p, v); }
};

// The waves' totals in front of this wave's, and all of them.
__device__ __forceinline__ uint32_t waves_before(const uint32_t *wt, int wave, uint32_t &all)
{
    uint32_t before = 0;
    all = 0;
#pragma unroll
    for (int w = 0; w < kTpWaves; ++w) {
        const uint32_t t = wt[w];
        before += w < wave ? t : 0u;
        all += t;
    }
    return before;
}

// dsts is read (the address words) and written (the dmac bytes) by different
// threads: no __restrict__.
__global__ void __launch_bounds__(kTpThreads)
k_tx_pump_plan(const uint32_t *__restrict__ tab, uint32_t *dsts, const uint8_t *__restrict__ afs,
               uint32_t ndst, const uint2 *__restrict__ desc, uint32_t n,
               const uint32_t *__restrict__ socks, uint32_t ns, const uint32_t *__restrict__ eng,
               uint8_t *sol_base, const uint64_t *__restrict__ sol_off, uint32_t m,
               uint32_t sol_slot_bytes, uint8_t *__restrict__ state, uint32_t *__restrict__ miss_list,
               unsigned long long *__restrict__ miss_count, uint8_t *__restrict__ hold,
               uint32_t *__restrict__ held_list, unsigned long long *__restrict__ held_count,
               uint16_t *__restrict__ sol_len, unsigned long long *__restrict__ sol_built)
{
    __shared__ uint32_t set[kTpSetWords];
    __shared__ uint32_t where[kTpReach];
    __shared__ uint32_t lmiss[kTpReach];
    __shared__ uint8_t lstate[kTpReach];
    __shared__ uint32_t wt[2][kTpWaves];
    __shared__ uint32_t nbuilt;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t w0 = (uint32_t)wave * kTpWaveSpan;
    const PumpWords w{};

    const uint32_t setw = ndst ? 2u * tn::set_slots(ndst) : 0u; // <= kTpSetWords
    for (uint32_t k = threadIdx.x; k < setw; k += kTpThreads)
        set[k] = 0u;
    if (threadIdx.x == 0)
        nbuilt = 0u;
    __syncthreads();

    // A: the lookup, dmac, the state byte; a miss joins the set
    const uint32_t cap = ndst ? tn::tab_cap(w, tab) : 0u;
#pragma unroll 1
    for (int step = 0; step < kTpSteps; ++step) {
        const uint32_t k = w0 + 64u * step + lane;
        if (k < ndst)
            tp::dst_find(w, tab, cap, dsts, afs, ndst, k, set, lstate, where);
    }
    __syncthreads();
    // B: the misses that did not win
#pragma unroll 1
    for (int step = 0; step < kTpSteps; ++step) {
        const uint32_t k = w0 + 64u * step + lane;
        if (k < ndst)
            tp::dst_mark(w, ndst, k, set, lstate, where);
    }
    __syncthreads();
    // C: the state bytes out; this wave's MISS and HELD counts
    uint32_t nmiss = 0, nheld = 0; // wave-uniform
    uint32_t hc[kTpSteps];
#pragma unroll
    for (int step = 0; step < kTpSteps; ++step) {
        const uint32_t k = w0 + 64u * step + lane;
        uint32_t s = ~0u;
        if (k < ndst) {
            s = lstate[k];
            state[k] = (uint8_t)s;
        }
        nmiss += (uint32_t)__builtin_popcountll(__ballot(s == tn::kMiss));

        uint32_t h = ~0u; // (no code)
        if (k < n) {
            const uint2 dd = desc[k];
            const txb::Desc d = txb::desc_of(dd.x, dd.y);
            const bool sock_in = d.sock < ns, dst_in = d.dst < ndst;
            const uint32_t s0 = sock_in ? socks[txb::kSockWords * d.sock] : 0u;
            const uint32_t daf = dst_in ? afs[d.dst] : 0u, dst = dst_in ? lstate[d.dst] : 0u;
            h = tn::hold_of(sock_in, s0, dst_in, daf, dst);
            hold[k] = (uint8_t)h;
        }
        hc[step] = h;
        nheld += (uint32_t)__builtin_popcountll(__ballot(h == tn::kThHeld));
    }
    if (lane == 0) {
        wt[0][wave] = nmiss;
        wt[1][wave] = nheld;
    }
    __syncthreads();
    // D: the two lists, the matches of the waves before this one first
    uint32_t miss_all, held_all;
    uint32_t at_m = waves_before(wt[0], wave, miss_all);
    uint32_t at_h = waves_before(wt[1], wave, held_all);
#pragma unroll
    for (int step = 0; step < kTpSteps; ++step) {
        const uint32_t k = w0 + 64u * step + lane;
        const bool miss = k < ndst && lstate[k] == tn::kMiss;
        const uint64_t bm = __ballot(miss);
        const uint32_t jm = at_m + mbcnt64(bm);
        if (miss && jm < ndst) { // (always: a rank among ndst entries)
            miss_list[jm] = k;
            lmiss[jm] = k;
        }
        at_m += (uint32_t)__builtin_popcountll(bm);

        const bool held = hc[step] == tn::kThHeld;
        const uint64_t bh = __ballot(held);
        const uint32_t jh = at_h + mbcnt64(bh);
        if (held && jh < n)
            held_list[jh] = k;
        at_h += (uint32_t)__builtin_popcountll(bh);
    }
    if (threadIdx.x == 0) {
        *miss_count = miss_all;
        *held_count = held_all;
    }
    __syncthreads();
    // E: the solicitations (k_tx_solicit_build's lines over the LDS list)
    const uint32_t lim = miss_all < m ? miss_all : m;
    const GlobalMem mem{};
    uint32_t nb = 0;
#pragma unroll 1
    for (uint64_t j = threadIdx.x; j < m; j += kTpThreads) { // (64 bits: j + 1024 never wraps below m)
        uint32_t len = 0;
        if (j < lim) {
            const uint32_t idx = lmiss[j]; // < ndst
            const uint32_t *t = dsts + txb::kDstWords * idx;
            const uint32_t a[4] = {t[0], t[1], t[2], t[3]};
            len = tn::solicit(mem, a, afs[idx], eng, (uint64_t)(uintptr_t)sol_base + sol_off[j],
                              sol_slot_bytes);
        }
        sol_len[j] = (uint16_t)len;
        nb += len != 0u;
    }
    nb = group_sum<64>(nb);
    if (lane == 0 && nb)
        atomicAdd(&nbuilt, nb); // (LDS)
    __syncthreads();
    if (threadIdx.x == 0)
        *sol_built = nbuilt;
}

} // namespace

hipError_t launch_tx_pump_plan(const void *tab, void *dsts, const uint8_t *afs, uint32_t ndst,
                               const void *desc, uint32_t n, const void *socks, uint32_t ns,
                               const void *eng, void *sol_base, const uint64_t *sol_off, uint32_t m,
                               uint32_t sol_slot_bytes, const TxPumpArrays &o, hipStream_t st)
{
    if (n > tp::kSmall || ndst > tp::kSmallDst || m > tp::kSmallDst)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_tx_pump_plan, dim3(1), dim3(kTpThreads), 0, st, (const uint32_t *)tab,
                       (uint32_t *)dsts, afs, ndst, (const uint2 *)desc, n, (const uint32_t *)socks,
                       ns, (const uint32_t *)eng, (uint8_t *)sol_base, sol_off, m, sol_slot_bytes,
                       o.state, o.miss_list, (unsigned long long *)o.miss_count, o.hold, o.held_list,
                       (unsigned long long *)o.held_count, o.sol_len,
                       (unsigned long long *)o.sol_built);
    return hipGetLastError();
}

} // namespace wc
