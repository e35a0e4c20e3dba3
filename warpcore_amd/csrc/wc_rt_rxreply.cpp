// wc_rt_rxreply.cpp -- RX replies (wc_rx_engine_check, wc_rx_reply_plan,
// wc_rx_reply_build): the table check on the host, the plan launch with its
// reply list (wc_rx_select's three launches over the action bytes), and the
// one launch that writes the reply frames.

#include "wc_rt.h"
#include "wc_rx_reply.h"

using namespace wc::rt;
namespace rr = wc::rr;

static_assert(sizeof(struct wc_rx_ifaddr) == 4 * rr::kIfaddrWords, "the entry as dwords");
static_assert(sizeof(struct wc_rx_engine) == 4 * rr::kEngineWords, "the table as dwords");
static_assert(WC_RX_MAX_IFADDR == rr::kMaxIfaddr && WC_RR_MASK_REPLY == rr::kMaskReply &&
                  WC_RR_UNREACH_PROTO4 == rr::kUnreachProto4 && WC_RR_ECHO4 == rr::kEcho4,
              "header and kernels agree");

extern "C" {

int wc_rx_engine_check(const struct wc_rx_engine *e)
{
    if (!e || e->naddr > WC_RX_MAX_IFADDR || e->mtu < 68)
        return WC_EINVAL;
    bool seen4 = false;
    for (uint32_t k = 0; k < e->naddr; ++k) {
        const uint8_t af = e->addr[k].af;
        if (af != 4 && af != 6)
            return WC_EINVAL;
        if (af == 6 && seen4) // IPv6 entries first (ifaddr.c:94-146)
            return WC_EINVAL;
        seen4 = seen4 || af == 4;
    }
    return WC_OK;
}

int wc_rx_reply_plan(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len,
                     uint64_t n, const uint8_t *d_verdict, const uint8_t *d_sock,
                     const struct wc_rx_engine *d_eng, uint32_t slot_bytes, uint8_t *d_action,
                     uint16_t *d_reply_len, uint32_t *d_list, uint64_t *d_count, void *d_scratch,
                     void *stream)
{
    if (n > kRxListMax || (d_list != nullptr) != (d_count != nullptr))
        return WC_EINVAL;
    if (n == 0) // an empty batch: a zero count
        return rx_zero_counts(d_count, nullptr, (hipStream_t)stream);
    if (slot_bytes > 65535u || !d_base || !d_off || !d_frame_len || !d_verdict || !d_eng ||
        ((uintptr_t)d_eng & 3u) || !d_action || !d_reply_len)
        return WC_EINVAL;
    if (!rx_scratch_ok(d_list != nullptr, d_scratch))
        return WC_EINVAL;
    Ready R;
    if (R.rc)
        return R.rc;
    hipError_t e = wc::launch_rx_reply_plan(d_base, d_off, d_frame_len, n, d_verdict, d_sock, d_eng,
                                            slot_bytes, d_action, d_reply_len, R.C.nt != 0,
                                            (hipStream_t)stream);
    if (e == hipSuccess && d_list)
        e = wc::launch_rx_select(d_action, n, WC_RR_MASK_REPLY, d_list, d_count, d_scratch,
                                 (hipStream_t)stream);
    return hip_err(e);
}

int wc_rx_reply_build(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len,
                      uint64_t n, const uint8_t *d_action, const uint32_t *d_list,
                      const uint64_t *d_count, const struct wc_rx_engine *d_eng, void *d_out_base,
                      const uint64_t *d_out_off, uint32_t m, uint32_t slot_bytes,
                      const uint16_t *d_ip_id, uint16_t *d_out_len, uint64_t *d_built, void *stream)
{
    const bool ptrs = rx_build_ptrs_ok(d_base, d_off, d_frame_len, d_action, d_list, d_count, d_eng,
                                       d_out_base, d_out_off);
    return rx_list_build(n, m, slot_bytes, ptrs, d_out_len, d_built, (hipStream_t)stream, [&](int cus) {
        return wc::launch_rx_reply_build(d_base, d_off, d_frame_len, n, d_action, d_list, d_count,
                                         d_eng, d_out_base, d_out_off, m, slot_bytes, d_ip_id,
                                         d_out_len, d_built, cus, (hipStream_t)stream);
    });
}

} // extern "C"
