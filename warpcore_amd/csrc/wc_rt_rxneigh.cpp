// wc_rt_rxneigh.cpp -- RX neighbours (wc_rx_neigh_plan, wc_rx_neigh_updates,
// wc_rx_neigh_build): the plan launch with its two lists (wc_rx_select's three
// launches each, one after the other through the one scratch), and the one
// launch each that writes the cache-update records and the reply frames
// (DESIGN.md section 4.10).

#include "wc_rt.h"
#include "wc_rx_neigh.h"

using namespace wc::rt;
namespace rn = wc::rn;

static_assert(sizeof(struct wc_neigh_update) == 24, "the record as six dwords");
static_assert(WC_RN_NONE == rn::kNone && WC_RN_MALFORMED == rn::kMalformed &&
                  WC_RN_UPDATE4 == rn::kUpdate4 && WC_RN_ARP_IS_AT == rn::kArpIsAt &&
                  WC_RN_NADV == rn::kNadv && WC_RN_UPDATE6 == rn::kUpdate6 &&
                  WC_RN_MASK_REPLY == rn::kMaskReply && WC_RN_MASK_UPDATE == rn::kMaskUpdate &&
                  WC_RR_HOST == wc::rr::kHost,
              "header and kernels agree");
static_assert(rn::kMaskReply == ((1u << rn::kArpIsAt) | (1u << rn::kNadv)) &&
                  rn::kMaskUpdate == ((1u << rn::kUpdate4) | (1u << rn::kUpdate6) | rn::kMaskReply),
              "the masks are the codes' bits");

extern "C" {

int wc_rx_neigh_plan(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len,
                     uint64_t n, const uint8_t *d_action, const struct wc_rx_engine *d_eng,
                     uint8_t *d_nact, uint32_t *d_rlist, uint64_t *d_rcount, uint32_t *d_ulist,
                     uint64_t *d_ucount, void *d_scratch, void *stream)
{
    if ((d_rlist != nullptr) != (d_rcount != nullptr) || (d_ulist != nullptr) != (d_ucount != nullptr))
        return WC_EINVAL;
    if (n > kRxListMax)
        return WC_EINVAL;
    hipStream_t st = (hipStream_t)stream;
    if (n == 0) // an empty batch: zero counts
        return rx_zero_counts(d_rcount, d_ucount, st);
    if (!d_base || !d_off || !d_frame_len || !d_action || !d_eng || ((uintptr_t)d_eng & 3u) || !d_nact)
        return WC_EINVAL;
    if (!rx_scratch_ok(d_rlist || d_ulist, d_scratch))
        return WC_EINVAL;
    Ready R;
    if (R.rc)
        return R.rc;
    hipError_t e = wc::launch_rx_neigh_plan(d_base, d_off, d_frame_len, n, d_action, d_eng, d_nact, st);
    if (e == hipSuccess && d_rlist)
        e = wc::launch_rx_select(d_nact, n, WC_RN_MASK_REPLY, d_rlist, d_rcount, d_scratch, st);
    if (e == hipSuccess && d_ulist)
        e = wc::launch_rx_select(d_nact, n, WC_RN_MASK_UPDATE, d_ulist, d_ucount, d_scratch, st);
    return hip_err(e);
}

int wc_rx_neigh_updates(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len,
                        uint64_t n, const uint8_t *d_nact, const uint32_t *d_list,
                        const uint64_t *d_count, uint32_t m, struct wc_neigh_update *d_upd,
                        void *stream)
{
    if (n > kRxListMax)
        return WC_EINVAL;
    if (m != 0 && !rx_updates_ptrs_ok(d_base, d_off, d_frame_len, n, d_nact, d_list, d_count, d_upd))
        return WC_EINVAL;
    if (m == 0)
        return WC_OK;
    Ready R;
    if (R.rc)
        return R.rc;
    hipError_t e;
    if (n == 0) // no frame, no record
        e = hipMemsetAsync(d_upd, 0, sizeof(struct wc_neigh_update) * (size_t)m, (hipStream_t)stream);
    else
        e = wc::launch_rx_neigh_updates(d_base, d_off, d_frame_len, n, d_nact, d_list, d_count, m,
                                        d_upd, R.D->cus, (hipStream_t)stream);
    return hip_err(e);
}

int wc_rx_neigh_build(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len,
                      uint64_t n, const uint8_t *d_nact, const uint32_t *d_list,
                      const uint64_t *d_count, const struct wc_rx_engine *d_eng, void *d_out_base,
                      const uint64_t *d_out_off, uint32_t m, uint32_t slot_bytes,
                      uint16_t *d_out_len, uint64_t *d_built, void *stream)
{
    const bool ptrs = rx_build_ptrs_ok(d_base, d_off, d_frame_len, d_nact, d_list, d_count, d_eng,
                                       d_out_base, d_out_off);
    return rx_list_build(n, m, slot_bytes, ptrs, d_out_len, d_built, (hipStream_t)stream, [&](int cus) {
        return wc::launch_rx_neigh_build(d_base, d_off, d_frame_len, n, d_nact, d_list, d_count, d_eng,
                                         d_out_base, d_out_off, m, slot_bytes, d_out_len, d_built,
                                         cus, (hipStream_t)stream);
    });
}

} // extern "C"
