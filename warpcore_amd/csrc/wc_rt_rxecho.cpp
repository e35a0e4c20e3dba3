// wc_rt_rxecho.cpp -- RX echo (wc_rx_echo): the argument checks and the one
// launch of wc_k_rxecho.hip.  No scratch, no library
// lock, no second path: the kernel takes every n and every m.

#include "wc_rt.h"
#include "wc_rx_echo.h"

using namespace wc::rt;
namespace re = wc::re;

static_assert(WC_EC_ECHO == re::kEcho && WC_EC_NONE == re::kNone && WC_EC_SHORT == re::kShort &&
                  WC_EC_NO_ROOM == re::kNoRoom && WC_EC_STALE == re::kStale &&
                  WC_ECHO_OFF == re::kOff && WC_RX_ECHO_MAX == re::kMax &&
                  WC_RX_DEMUX_MAX_SOCKS == re::kMaxSocks,
              "header and kernel agree");
static_assert(sizeof(struct wc_rx_echo_out) == 8 * sizeof(void *), "eight pointers");
static_assert(sizeof(struct wc_tx_desc) == 8 && sizeof(struct wc_tx_dst) == 24 &&
                  sizeof(struct wc_rx_record) == 16,
              "the kernel's dword views");

extern "C" {

int wc_rx_echo(const void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len, uint64_t n,
               const struct wc_rx_record *d_rec, const uint32_t *d_list, const uint64_t *d_start,
               const uint16_t *d_map, uint32_t ns, const uint16_t *d_ip_id, void *d_out_base,
               const uint64_t *d_out_off, uint32_t out_slot_bytes, uint32_t m,
               const struct wc_rx_echo_out *out, void *stream)
{
    if (!out || !out->count)
        return WC_EINVAL;
    if (n > kRxListMax || ns > WC_RX_DEMUX_MAX_SOCKS || m > WC_RX_ECHO_MAX || out_slot_bytes > 65535u)
        return WC_EINVAL;
    const struct wc_rx_echo_out &o = *out;
    auto misaligned = [](const void *p, uintptr_t a) { return ((uintptr_t)p & (a - 1u)) != 0; };
    if (misaligned(d_rec, 16) || misaligned(d_out_off, 8))
        return WC_EINVAL;
    if (m != 0) {
        if (!o.desc || !o.dsts || !o.af || !o.status)
            return WC_EINVAL;
        if (misaligned(o.desc, 8) || misaligned(o.dsts, 4) || misaligned(o.tx_off, 8))
            return WC_EINVAL;
        const bool copy = d_out_base && d_out_off && !o.tx_off;
        const bool in_place = !d_out_base && !d_out_off && o.tx_off;
        if (!copy && !in_place)
            return WC_EINVAL;
    }
    const bool rx = n != 0 && ns != 0;
    if (rx && (!d_base || !d_off || !d_frame_len || !d_rec || !d_list || !d_start || !d_map))
        return WC_EINVAL;

    Ready R;
    if (R.rc)
        return R.rc;
    const wc::RxEchoArgs a{(const uint8_t *)d_base, d_off, d_frame_len, n, d_rec, d_list, d_start,
                           d_map, ns, d_ip_id, (uint8_t *)d_out_base, d_out_off, out_slot_bytes, m,
                           (uint32_t *)o.desc, (uint32_t *)o.dsts, o.af, o.status, o.src,
                           // (m = 0: the kernel leaves before it asks for the mode)
                           o.tx_off, o.count, o.skipped};
    return hip_err(wc::launch_rx_echo(a, (hipStream_t)stream));
}

} // extern "C"
