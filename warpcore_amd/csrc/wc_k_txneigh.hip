// wc_k_txneigh.hip -- the TX neighbour kernels on gfx950: the neighbour cache
// as a device-resident open-addressed table (neighbor.c's hash), neighbor_update
// for a whole wc_rx_neigh_updates array, who_has's lookup for a whole
// destination table with one solicitation per distinct unresolved address, the
// per-frame READY / HELD plan, and the ARP who-has and neighbour solicitation
// frames arp_who_has and icmp6_nsol write.  DESIGN.md section 4.11.  The table
// layout, the hash, every probe step, the chain and the frame words are
// wc_tx_neigh.h's; this file holds the grids and the device's Words.
//
// One lane per record / destination / frame / list entry, workgroups of 256, the
// grid no larger than the device holds at once, each lane striding.
//   k_neigh_tab_init      zero words, then magic and cap.
//   k_neigh_apply_claim   record j: hash, linear probe, compare-and-swap of an
//                         empty state word, atomicMax(last, j + 1); the entry
//                         index goes to scratch[j].  One atomicAdd per workgroup
//                         with a dropped record.
//   k_neigh_apply_commit  the record whose j + 1 is its entry's last writes it.
//   k_tx_resolve_find     destination k: the lookup, dmac, the state byte; a
//                         miss claims or joins a slot of the scratch set with
//                         atomicMax(~k), so the lowest index wins.
//   k_tx_resolve_mark     a miss that did not win is MISS_DUP.
//   k_tx_hold_plan        the chain over descriptor, socket word and the
//                         destination's state and family bytes.
//   k_tx_solicit_build    the list kernels' frame (k_rx_neigh_build's).
// What lanes of one launch tell each other goes through atomics on the table's
// or the set's own words, read back with agent-scope loads (Words::ld_now);
// everything else a lane reads was written before the launch.  No lane waits
// for another: every loop is bounded by cap (the set: by its slots), and the
// result is the same however the lanes interleave (wc_tx_neigh.h says why).
// Frame stores are plain vector stores (txb::store_words).
// Roofline: latency -- a hash and a few dependent loads per lane.
#include "wc_rx_hdr.h"
#include "wc_tx_neigh.h"

namespace wc {
namespace {

constexpr uint32_t kTnBlock = 256;

// (wc_tx_neigh.h's Words on the device: DevWords, wc_device.h)

__global__ void __launch_bounds__(kTnBlock)
k_neigh_tab_init(uint32_t *__restrict__ tab, uint32_t cap)
{
    const uint64_t words = tn::kHdrWords + (uint64_t)tn::kEntWords * cap;
    const uint64_t S = (uint64_t)gridDim.x * kTnBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kTnBlock + threadIdx.x; i < words; i += S)
        tab[i] = i == 0 ? tn::kTabMagic : i == 1 ? cap : 0u;
}

__global__ void __launch_bounds__(kTnBlock)
k_neigh_apply_claim(uint32_t *tab, const uint32_t *__restrict__ upd,
                    const unsigned long long *__restrict__ count, uint32_t m,
                    uint32_t *__restrict__ scratch, unsigned long long *__restrict__ dropped)
{
    const DevWords w{};
    const uint32_t lim = (uint32_t)list_limit(count, m);
    const uint32_t cap = tn::tab_cap(w, tab);
    uint32_t ndrop = 0;
    const uint64_t S = (uint64_t)gridDim.x * kTnBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kTnBlock + threadIdx.x; j < lim; j += S) {
        bool drop;
        scratch[j] = tn::apply_claim(w, tab, cap, upd, lim, (uint32_t)j, drop);
        ndrop += drop;
    }
    if (dropped) // (uniform: a kernel argument)
        block_count_add<kTnBlock / 64>(group_sum<64>(ndrop), dropped);
}

__global__ void __launch_bounds__(kTnBlock)
k_neigh_apply_commit(uint32_t *tab, const uint32_t *__restrict__ upd,
                     const unsigned long long *__restrict__ count, uint32_t m,
                     const uint32_t *__restrict__ scratch)
{
    const DevWords w{};
    const uint32_t lim = (uint32_t)list_limit(count, m);
    const uint32_t cap = tn::tab_cap(w, tab);
    const uint64_t S = (uint64_t)gridDim.x * kTnBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kTnBlock + threadIdx.x; j < lim; j += S)
        tn::apply_commit(w, tab, cap, upd, (uint32_t)j, scratch[j]);
}

// dsts is read (the address words) and written (the dmac bytes) by different
// lanes: no __restrict__.
__global__ void __launch_bounds__(kTnBlock)
k_tx_resolve_find(const uint32_t *__restrict__ tab, uint32_t *dsts, const uint8_t *__restrict__ afs,
                  uint32_t ndst, uint32_t *set, uint32_t slots, uint8_t *__restrict__ state,
                  uint32_t *__restrict__ where)
{
    const DevWords w{};
    const uint32_t cap = tn::tab_cap(w, tab);
    const uint32_t S = gridDim.x * kTnBlock;
    for (uint32_t k = blockIdx.x * kTnBlock + threadIdx.x; k < ndst; k += S)
        tn::resolve_find(w, tab, cap, dsts, afs, ndst, k, set, slots, state, where);
}

__global__ void __launch_bounds__(kTnBlock)
k_tx_resolve_mark(uint32_t ndst, const uint32_t *__restrict__ set, uint32_t slots,
                  uint8_t *__restrict__ state, const uint32_t *__restrict__ where)
{
    const DevWords w{};
    const uint32_t S = gridDim.x * kTnBlock;
    for (uint32_t k = blockIdx.x * kTnBlock + threadIdx.x; k < ndst; k += S)
        tn::resolve_mark(w, k, set, slots, state, where);
}

__global__ void __launch_bounds__(kTnBlock)
k_tx_hold_plan(const uint2 *__restrict__ desc, uint64_t n, const uint32_t *__restrict__ socks,
               uint32_t ns, const uint8_t *__restrict__ state, const uint8_t *__restrict__ afs,
               uint32_t ndst, uint8_t *__restrict__ hold)
{
    const uint64_t S = (uint64_t)gridDim.x * kTnBlock;
    for (uint64_t i = (uint64_t)blockIdx.x * kTnBlock + threadIdx.x; i < n; i += S) {
        const uint2 dd = desc[i];
        const txb::Desc d = txb::desc_of(dd.x, dd.y);
        const bool sock_in = d.sock < ns, dst_in = d.dst < ndst;
        const uint32_t w0 = sock_in ? socks[txb::kSockWords * d.sock] : 0u;
        const uint32_t daf = dst_in ? afs[d.dst] : 0u, dst = dst_in ? state[d.dst] : 0u;
        hold[i] = (uint8_t)tn::hold_of(sock_in, w0, dst_in, daf, dst);
    }
}

__global__ void __launch_bounds__(kTnBlock)
k_tx_solicit_build(const uint32_t *__restrict__ dsts, const uint8_t *__restrict__ afs, uint32_t ndst,
                   const uint32_t *__restrict__ list, const unsigned long long *__restrict__ count,
                   const uint32_t *__restrict__ eng, uint8_t *out_base,
                   const uint64_t *__restrict__ out_off, uint32_t m, uint32_t slot_bytes,
                   uint16_t *__restrict__ out_len, unsigned long long *__restrict__ built)
{
    const uint64_t lim = list_limit(count, m);
    const GlobalMem mem{};
    uint32_t nbuilt = 0;
    const uint64_t S = (uint64_t)gridDim.x * kTnBlock;
    for (uint64_t j = (uint64_t)blockIdx.x * kTnBlock + threadIdx.x; j < m; j += S) {
        const uint64_t idx = list_entry(list, j, lim);
        uint32_t len = 0;
        if (idx < ndst) {
            const uint32_t *t = dsts + txb::kDstWords * idx;
            const uint32_t a[4] = {t[0], t[1], t[2], t[3]};
            len = tn::solicit(mem, a, afs[idx], eng, (uint64_t)(uintptr_t)out_base + out_off[j],
                              slot_bytes);
        }
        out_len[j] = (uint16_t)len;
        nbuilt += len != 0u;
    }
    block_count_add<kTnBlock / 64>(group_sum<64>(nbuilt), built);
}

} // namespace

hipError_t launch_neigh_tab_init(void *tab, uint32_t cap, int cus, hipStream_t st)
{
    const uint32_t words = tn::kHdrWords + tn::kEntWords * cap;
    const int grid = list_grid<k_neigh_tab_init, kTnBlock, kTnBlock>(words, cus);
    hipLaunchKernelGGL(k_neigh_tab_init, dim3(grid), dim3(kTnBlock), 0, st, (uint32_t *)tab, cap);
    return hipGetLastError();
}

hipError_t launch_neigh_apply(void *tab, const void *upd, const uint64_t *count, uint32_t m,
                              uint64_t *dropped, void *scratch, int cus, hipStream_t st)
{
    int grid = list_grid<k_neigh_apply_claim, kTnBlock, kTnBlock>(m, cus);
    hipLaunchKernelGGL(k_neigh_apply_claim, dim3(grid), dim3(kTnBlock), 0, st, (uint32_t *)tab,
                       (const uint32_t *)upd, (const unsigned long long *)count, m,
                       (uint32_t *)scratch, (unsigned long long *)dropped);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    grid = list_grid<k_neigh_apply_commit, kTnBlock, kTnBlock>(m, cus);
    hipLaunchKernelGGL(k_neigh_apply_commit, dim3(grid), dim3(kTnBlock), 0, st, (uint32_t *)tab,
                       (const uint32_t *)upd, (const unsigned long long *)count, m,
                       (const uint32_t *)scratch);
    return hipGetLastError();
}

uint64_t tx_resolve_set_bytes(uint32_t ndst)
{
    return ndst ? 4ull * (2ull * tn::set_slots(ndst) + ndst) : 0ull;
}

hipError_t launch_tx_resolve(const void *tab, void *dsts, const uint8_t *afs, uint32_t ndst,
                             uint8_t *state, void *scratch, int cus, hipStream_t st)
{
    const uint32_t slots = tn::set_slots(ndst);
    uint32_t *set = (uint32_t *)scratch, *where = set + 2u * slots;
    hipError_t e = hipMemsetAsync(set, 0, 8ull * slots, st);
    if (e != hipSuccess)
        return e;
    int grid = list_grid<k_tx_resolve_find, kTnBlock, kTnBlock>(ndst, cus);
    hipLaunchKernelGGL(k_tx_resolve_find, dim3(grid), dim3(kTnBlock), 0, st, (const uint32_t *)tab,
                       (uint32_t *)dsts, afs, ndst, set, slots, state, where);
    e = hipGetLastError();
    if (e != hipSuccess)
        return e;
    grid = list_grid<k_tx_resolve_mark, kTnBlock, kTnBlock>(ndst, cus);
    hipLaunchKernelGGL(k_tx_resolve_mark, dim3(grid), dim3(kTnBlock), 0, st, ndst,
                       (const uint32_t *)set, slots, state, (const uint32_t *)where);
    return hipGetLastError();
}

hipError_t launch_tx_hold_plan(const void *desc, uint64_t n, const void *socks, uint32_t ns,
                               const uint8_t *state, const uint8_t *afs, uint32_t ndst,
                               uint8_t *hold, int cus, hipStream_t st)
{
    const uint32_t m = (uint32_t)std::min<uint64_t>(n, 0xFFFFFFFFull);
    const int grid = list_grid<k_tx_hold_plan, kTnBlock, kTnBlock>(m, cus);
    hipLaunchKernelGGL(k_tx_hold_plan, dim3(grid), dim3(kTnBlock), 0, st, (const uint2 *)desc, n,
                       (const uint32_t *)socks, ns, state, afs, ndst, hold);
    return hipGetLastError();
}

hipError_t launch_tx_solicit_build(const void *dsts, const uint8_t *afs, uint32_t ndst,
                                   const uint32_t *list, const uint64_t *count, const void *eng,
                                   void *out_base, const uint64_t *out_off, uint32_t m,
                                   uint32_t slot_bytes, uint16_t *out_len, uint64_t *built, int cus,
                                   hipStream_t st)
{
    const int grid = list_grid<k_tx_solicit_build, kTnBlock, kTnBlock>(m, cus);
    hipLaunchKernelGGL(k_tx_solicit_build, dim3(grid), dim3(kTnBlock), 0, st, (const uint32_t *)dsts,
                       afs, ndst, list, (const unsigned long long *)count, (const uint32_t *)eng,
                       (uint8_t *)out_base, out_off, m, slot_bytes, out_len,
                       (unsigned long long *)built);
    return hipGetLastError();
}

} // namespace wc
