// wc_rt_tx.cpp -- the TX seal (wc_tx_seal_ragged, wc_tx_seal_host): one
// asynchronous launch of k_tx_seal for device-resident frames; for host
// memory the kernel's no-store mode over the host paths of wc_rt_host.cpp,
// then the raw stores by the calling thread.

#include "wc_rt.h"

#include <cstring>
#include <new>

using namespace wc::rt;

extern "C" {

int wc_tx_seal_ragged(void *d_base, const uint64_t *d_off, const uint16_t *d_frame_len,
                      uint64_t n, uint32_t flags, uint8_t *d_status, uint16_t *d_out_ip_hdr,
                      uint16_t *d_out_udp, uint64_t *d_errors, void *stream)
{
    if (n == 0)
        return WC_OK;
    if (flags & ~(uint32_t)(WC_TX_ZERO_UDP_CKSUM | WC_TX_NO_STORE))
        return WC_EINVAL;
    if ((flags & WC_TX_NO_STORE) && (!d_out_ip_hdr || !d_out_udp))
        return WC_EINVAL;
    if (!d_base || !d_off || !d_frame_len || !d_status)
        return WC_EINVAL;
    Device *D = nullptr;
    Config C;
    int rc = ensure_device(&D, &C);
    if (rc)
        return rc;
    static_assert(WC_TX_ZERO_UDP_CKSUM == wc::kTxZeroUdp && WC_TX_NO_STORE == wc::kTxNoStore,
                  "the kernel's flags are the ABI's");
    return hip_err(wc::launch_tx_seal(d_base, d_off, d_frame_len, n, flags, d_status,
                                      d_out_ip_hdr, d_out_udp, d_errors, C.nt != 0,
                                      (hipStream_t)stream));
}

int wc_tx_seal_host(void *h_base, uint64_t h_bytes, const uint64_t *h_off,
                    const uint16_t *h_frame_len, uint64_t n, uint32_t flags, uint8_t *h_status,
                    uint64_t *h_errors)
{
    if (n == 0) {
        if (h_errors)
            *h_errors = 0;
        return WC_OK;
    }
    if (flags & ~(uint32_t)WC_TX_ZERO_UDP_CKSUM) // (WC_TX_NO_STORE: the device call's)
        return WC_EINVAL;
    if (!h_base || !h_off || !h_frame_len || !h_status)
        return WC_EINVAL;
    // Both values of every frame, computed on the device with no frame byte
    // written there (host_batch checks every frame against the region).
    uint16_t *vals = new (std::nothrow) uint16_t[2 * n];
    if (!vals)
        return WC_ENOMEM;
    uint16_t *udp = vals, *iph = vals + n;
    const bool zero_udp = flags & WC_TX_ZERO_UDP_CKSUM;
    const int rc = host_batch(h_base, h_bytes, h_off, h_frame_len, n,
                              {{(uint8_t *)udp, (uint8_t *)iph, h_status}},
                              zero_udp ? kKindTxZero : kKindTx);
    if (rc == WC_OK) {
        // The stores of mk_ip4_hdr and udp_tx (ip4.c:184-186, udp.c:209-213),
        // by the status: a frame that has one is IPv4 or IPv6 with its header
        // inside it, so its EtherType and IHL bytes are there to find the
        // fields by.
        uint8_t *hb = (uint8_t *)h_base;
        uint64_t errs = 0;
        for (uint64_t i = 0; i < n; ++i) {
            const uint8_t s = h_status[i];
            errs += WC_TX_IS_ERROR(s);
            if (s > WC_TX_IP_ONLY)
                continue;
            uint8_t *ip = hb + h_off[i] + 14;
            const bool v4 = ip[-2] == 0x08; // 0x0800, else 0x86DD
            if (v4)
                memcpy(ip + 10, &iph[i], 2);
            if (s != WC_TX_IP_ONLY)
                memcpy(ip + (v4 ? (ip[0] & 15u) * 4u : 40u) + 6, &udp[i], 2);
        }
        if (h_errors)
            *h_errors = errs;
    }
    delete[] vals;
    return rc;
}

} // extern "C"
