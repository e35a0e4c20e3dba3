// wc_rt_txneigh.cpp -- TX neighbours (wc_neigh_tab_*, wc_neigh_apply,
// wc_tx_resolve, wc_tx_hold_plan, wc_tx_solicit_build): the argument checks and
// launches of the device calls, and the two pure host calls over a host copy of
// the table, which run wc_tx_neigh.h's own lookup.

#include "wc_rt.h"
#include "wc_tx_neigh.h"

using namespace wc::rt;
namespace tn = wc::tn;

static_assert(WC_NEIGH_TAB_MIN_CAP == tn::kTabMinCap && WC_NEIGH_TAB_MAX_CAP == tn::kTabMaxCap,
              "header and kernels agree");
static_assert(WC_NR_READY == tn::kReady && WC_NR_BAD_AF == tn::kBadAf && WC_NR_MISS == tn::kMiss &&
                  WC_NR_MISS_DUP == tn::kMissDup && WC_NR_MASK_SOLICIT == tn::kMaskSolicit &&
                  WC_NR_MASK_MISS == tn::kMaskMiss && WC_TH_READY == tn::kThReady &&
                  WC_TH_MALFORMED == tn::kThMalformed && WC_TH_HELD == tn::kThHeld &&
                  WC_TH_MASK_HELD == tn::kMaskHeld,
              "header and kernels agree");
static_assert(tn::kMaskSolicit == (1u << tn::kMiss) &&
                  tn::kMaskMiss == ((1u << tn::kMiss) | (1u << tn::kMissDup)) &&
                  tn::kMaskHeld == (1u << tn::kThHeld),
              "the masks are the codes' bits");
static_assert(sizeof(struct wc_neigh_update) == 4 * tn::kUpdWords &&
                  sizeof(struct wc_tx_dst) == 4 * wc::txb::kDstWords &&
                  sizeof(struct wc_tx_sock) == 4 * wc::txb::kSockWords,
              "the records and entries as dwords");
static_assert(tn::kResolveMax == 65536u, "the TX build's ndst limit");
static_assert(tn::kApplyMax == 1u << 31, "neigh_apply_args_ok's limit");

namespace {

// A host copy of the table as words, or nullptr for one init did not write.
const uint32_t *host_tab(const void *h_tab, uint32_t *cap)
{
    if (!h_tab || ((uintptr_t)h_tab & 3u))
        return nullptr;
    const uint32_t *t = (const uint32_t *)h_tab;
    *cap = tn::tab_cap(tn::HostWords{}, t);
    return *cap ? t : nullptr;
}

} // namespace

extern "C" {

uint64_t wc_neigh_tab_bytes(uint32_t cap)
{
    return tn::tab_bytes(cap);
}

int wc_neigh_tab_init(void *d_tab, uint32_t cap, void *stream)
{
    if (!tn::cap_ok(cap) || !d_tab || ((uintptr_t)d_tab & 15u))
        return WC_EINVAL;
    Ready R;
    if (R.rc)
        return R.rc;
    return hip_err(wc::launch_neigh_tab_init(d_tab, cap, R.D->cus, (hipStream_t)stream));
}

uint64_t wc_neigh_apply_scratch(uint32_t m)
{
    return 4ull * m;
}

int wc_neigh_apply(void *d_tab, const struct wc_neigh_update *d_upd, const uint64_t *d_count,
                   uint32_t m, uint64_t *d_dropped, void *d_scratch, void *stream)
{
    if (m == 0)
        return WC_OK;
    if (!neigh_apply_args_ok(d_tab, d_upd, d_count, m, d_scratch))
        return WC_EINVAL;
    Ready R;
    if (R.rc)
        return R.rc;
    return hip_err(wc::launch_neigh_apply(d_tab, d_upd, d_count, m, d_dropped, d_scratch, R.D->cus,
                                          (hipStream_t)stream));
}

int wc_neigh_tab_lookup(const void *h_tab, uint8_t af, const uint8_t *addr, uint8_t mac[6])
{
    uint32_t cap = 0;
    const uint32_t *t = host_tab(h_tab, &cap);
    if (!t || !addr || !mac || (af != 4 && af != 6))
        return WC_EINVAL;
    uint32_t a[4] = {0u, 0u, 0u, 0u};
    memcpy(a, addr, af == 4 ? 4 : 16);
    uint32_t m0 = 0, m1 = 0;
    if (!tn::lookup(tn::HostWords{}, t, cap, tn::key_of(af, a[0], a[1], a[2], a[3]), m0, m1))
        return 0;
    memcpy(mac, &m0, 4);
    memcpy(mac + 4, &m1, 2);
    return 1;
}

int wc_neigh_tab_stats(const void *h_tab, uint32_t *cap, uint32_t *used)
{
    uint32_t c = 0;
    const uint32_t *t = host_tab(h_tab, &c);
    if (!t)
        return WC_EINVAL;
    uint32_t u = 0;
    for (uint32_t s = 0; s < c; ++s)
        u += *tn::tab_entry(t, s) == tn::kFull;
    if (cap)
        *cap = c;
    if (used)
        *used = u;
    return WC_OK;
}

uint64_t wc_tx_resolve_scratch(uint32_t ndst)
{
    if (ndst > tn::kResolveMax)
        return 0;
    // the set, then -- behind it on the stream -- the list's wc_rx_select
    return std::max<uint64_t>(wc::tx_resolve_set_bytes(ndst), wc::rxsel_scratch_bytes(ndst));
}

int wc_tx_resolve(const void *d_tab, struct wc_tx_dst *d_dsts, const uint8_t *d_af, uint32_t ndst,
                  uint8_t *d_state, uint32_t *d_list, uint64_t *d_count, void *d_scratch,
                  void *stream)
{
    if ((d_list != nullptr) != (d_count != nullptr) || ndst > tn::kResolveMax)
        return WC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (ndst == 0)
        return rx_zero_counts(d_count, nullptr, st);
    if (!tx_resolve_ptrs_ok(d_tab, d_dsts, d_af, d_state, d_scratch))
        return WC_EINVAL;
    Ready R;
    if (R.rc)
        return R.rc;
    hipError_t e = wc::launch_tx_resolve(d_tab, d_dsts, d_af, ndst, d_state, d_scratch, R.D->cus, st);
    if (e == hipSuccess && d_list)
        e = wc::launch_rx_select(d_state, ndst, WC_NR_MASK_SOLICIT, d_list, d_count, d_scratch, st);
    return hip_err(e);
}

int wc_tx_hold_plan(const struct wc_tx_desc *d_desc, uint64_t n, const struct wc_tx_sock *d_socks,
                    uint32_t ns, const uint8_t *d_state, const uint8_t *d_af, uint32_t ndst,
                    uint8_t *d_hold, uint32_t *d_list, uint64_t *d_count, void *d_scratch,
                    void *stream)
{
    if ((d_list != nullptr) != (d_count != nullptr))
        return WC_EINVAL;
    if (n > kRxListMax || ns > WC_TX_BUILD_MAX_SOCKS || ndst > tn::kResolveMax)
        return WC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0)
        return rx_zero_counts(d_count, nullptr, st);
    if (!tx_hold_ptrs_ok(d_desc, d_hold, d_socks, ns, d_state, d_af, ndst, d_list != nullptr,
                         d_scratch))
        return WC_EINVAL;
    Ready R;
    if (R.rc)
        return R.rc;
    hipError_t e = wc::launch_tx_hold_plan(d_desc, n, d_socks, ns, d_state, d_af, ndst, d_hold,
                                           R.D->cus, st);
    if (e == hipSuccess && d_list)
        e = wc::launch_rx_select(d_hold, n, WC_TH_MASK_HELD, d_list, d_count, d_scratch, st);
    return hip_err(e);
}

int wc_tx_solicit_build(const struct wc_tx_dst *d_dsts, const uint8_t *d_af, uint32_t ndst,
                        const uint32_t *d_list, const uint64_t *d_count,
                        const struct wc_rx_engine *d_eng, void *d_out_base,
                        const uint64_t *d_out_off, uint32_t m, uint32_t slot_bytes,
                        uint16_t *d_out_len, uint64_t *d_built, void *stream)
{
    if (ndst > tn::kResolveMax)
        return WC_EINVAL;
    const bool ptrs =
        tx_solicit_ptrs_ok(d_dsts, d_af, d_list, d_count, d_eng, d_out_base, d_out_off);
    return rx_list_build(ndst, m, slot_bytes, ptrs, d_out_len, d_built, (hipStream_t)stream,
                         [&](int cus) {
                             return wc::launch_tx_solicit_build(d_dsts, d_af, ndst, d_list, d_count,
                                                                d_eng, d_out_base, d_out_off, m,
                                                                slot_bytes, d_out_len, d_built, cus,
                                                                (hipStream_t)stream);
                         });
}

} // extern "C"
