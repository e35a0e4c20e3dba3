// wc_rt_tx.cpp -- the TX seal (wc_tx_seal_ragged, wc_tx_seal_host): one
// asynchronous launch of k_tx_seal for device-resident frames; for host
// memory the kernel's no-store mode over the host paths of wc_rt_host.cpp,
// then the raw stores by the calling thread.  And the
// TX build (wc_tx_socks_check, wc_tx_build_ragged, wc_tx_build_host): one
// asynchronous launch of k_tx_build; for host memory the calling thread writes
// the headers and the seal's host batch computes the two values (section 4.8).

#include "wc_rt.h"
#include "wc_tx_build.h"

#include <cstring>
#include <new>

using namespace wc::rt;

// The stores of mk_ip4_hdr and udp_tx (ip4.c:184-186, udp.c:209-213) into one
// frame, by its seal status: a frame that has one up to WC_TX_IP_ONLY is IPv4
// or IPv6 with its header inside it, so its EtherType and IHL bytes are there
// to find the fields by; any other frame is left as it is.
static void tx_store_sums(uint8_t *frame, uint8_t status, uint16_t iph, uint16_t udp)
{
    if (status > WC_TX_IP_ONLY)
        return;
    uint8_t *ip = frame + 14;
    const bool v4 = ip[-2] == 0x08; // 0x0800, else 0x86DD
    if (v4)
        memcpy(ip + 10, &iph, 2);
    if (status != WC_TX_IP_ONLY)
        memcpy(ip + (v4 ? (ip[0] & 15u) * 4u : 40u) + 6, &udp, 2);
}

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
    Ready R;
    if (R.rc)
        return R.rc;
    static_assert(WC_TX_ZERO_UDP_CKSUM == wc::kTxZeroUdp && WC_TX_NO_STORE == wc::kTxNoStore,
                  "the kernel's flags are the ABI's");
    return hip_err(wc::launch_tx_seal(d_base, d_off, d_frame_len, n, flags, d_status,
                                      d_out_ip_hdr, d_out_udp, d_errors, R.C.nt != 0,
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
        uint64_t errs = 0;
        for (uint64_t i = 0; i < n; ++i) {
            errs += WC_TX_IS_ERROR(h_status[i]);
            tx_store_sums((uint8_t *)h_base + h_off[i], h_status[i], iph[i], udp[i]);
        }
        if (h_errors)
            *h_errors = errs;
    }
    delete[] vals;
    return rc;
}

// --- TX build (wc_k_txbuild.hip, wc_tx_build.h) --------

namespace txb = wc::txb;
static_assert(sizeof(wc_tx_sock) == 4 * txb::kSockWords && sizeof(wc_tx_dst) == 4 * txb::kDstWords &&
                  sizeof(wc_tx_desc) == 8,
              "the kernel reads the ABI's structs as dwords");
static_assert(WC_TX_SOCK_CONNECTED == txb::kSockConnected && WC_TX_SOCK_ECN == txb::kSockEcn &&
                  WC_TX_MALFORMED == txb::kMalformed && WC_TX_TRUNCATED == txb::kTruncated &&
                  WC_TX_SEALED == txb::kSealed && WC_TX_SEALED_ZERO_UDP == txb::kSealedZeroUdp,
              "the kernel's codes are the ABI's");

int wc_tx_socks_check(const struct wc_tx_sock *socks, uint32_t ns)
{
    if (ns > WC_TX_BUILD_MAX_SOCKS || (ns && !socks))
        return WC_EINVAL;
    for (uint32_t i = 0; i < ns; ++i) {
        if (socks[i].af != 4 && socks[i].af != 6)
            return WC_EINVAL;
        if (socks[i].flags & ~(WC_TX_SOCK_CONNECTED | WC_TX_SOCK_ECN))
            return WC_EINVAL;
    }
    return WC_OK;
}

} // extern "C"

// The argument rules both build calls (and wc_tx_pump) share (n > 0), before a
// device is touched.
int wc::rt::tx_build_args(const void *base, const void *off, const void *desc, const void *socks,
                          uint32_t ns, const void *dsts, uint32_t ndst, const void *frame_len,
                          const void *status)
{
    if (!base || !off || !desc || !frame_len || !status)
        return WC_EINVAL;
    if ((ns && !socks) || (ndst && !dsts) || ns > WC_TX_BUILD_MAX_SOCKS || ndst > 65536u)
        return WC_EINVAL;
    if (((uintptr_t)desc & 7u) || ((uintptr_t)socks & 3u) || ((uintptr_t)dsts & 3u))
        return WC_EINVAL;
    return WC_OK;
}

extern "C" {

int wc_tx_build_ragged(void *d_base, const uint64_t *d_off, const struct wc_tx_desc *d_desc,
                       uint64_t n, const struct wc_tx_sock *d_socks, uint32_t ns,
                       const struct wc_tx_dst *d_dsts, uint32_t ndst, uint32_t slot_bytes,
                       uint32_t flags, uint16_t *d_frame_len, uint8_t *d_status,
                       uint16_t *d_out_ip_hdr, uint16_t *d_out_udp, uint64_t *d_errors,
                       void *stream)
{
    if (n == 0)
        return WC_OK;
    if (flags & ~(uint32_t)(WC_TX_ZERO_UDP_CKSUM | WC_TX_NO_STORE))
        return WC_EINVAL;
    if ((flags & WC_TX_NO_STORE) && (!d_out_ip_hdr || !d_out_udp))
        return WC_EINVAL;
    const int rc =
        tx_build_args(d_base, d_off, d_desc, d_socks, ns, d_dsts, ndst, d_frame_len, d_status);
    if (rc)
        return rc;
    Ready R;
    if (R.rc)
        return R.rc;
    return hip_err(wc::launch_tx_build(d_base, d_off, d_desc, n, d_socks, ns, d_dsts, ndst,
                                       slot_bytes, flags, d_frame_len, d_status, d_out_ip_hdr,
                                       d_out_udp, d_errors, R.C.nt != 0, (hipStream_t)stream));
}

namespace {

struct HostMem { // txb::store_headers' stores into host memory
    void st32(uint64_t a, uint32_t v) const { memcpy((void *)(uintptr_t)a, &v, 4); }
    void st16(uint64_t a, uint32_t v) const
    {
        const uint16_t x = (uint16_t)v;
        memcpy((void *)(uintptr_t)a, &x, 2);
    }
    void st8(uint64_t a, uint32_t v) const { *(uint8_t *)(uintptr_t)a = (uint8_t)v; }
};

// One frame's descriptor and table entries as the kernel reads them.
struct HostFrame {
    wc::txb::Desc d;
    wc::txb::Decide x;
    uint32_t w[wc::txb::kSockWords], t[wc::txb::kDstWords];
};

HostFrame host_frame(const wc_tx_desc *desc, uint64_t i, const wc_tx_sock *socks, uint32_t ns,
                     const wc_tx_dst *dsts, uint32_t ndst, uint32_t slot_bytes, bool zero_udp)
{
    HostFrame f{};
    uint32_t dw[2];
    memcpy(dw, &desc[i], 8);
    f.d = wc::txb::desc_of(dw[0], dw[1]);
    const bool sock_in = f.d.sock < ns, dst_in = f.d.dst < ndst;
    if (sock_in)
        memcpy(f.w, &socks[f.d.sock], sizeof f.w);
    if (dst_in)
        memcpy(f.t, &dsts[f.d.dst], sizeof f.t);
    f.x = wc::txb::decide(sock_in, f.w[0], dst_in, f.d.data_len, slot_bytes, zero_udp);
    return f;
}

} // namespace

int wc_tx_build_host(void *h_base, uint64_t h_bytes, const uint64_t *h_off,
                     const struct wc_tx_desc *h_desc, uint64_t n, const struct wc_tx_sock *h_socks,
                     uint32_t ns, const struct wc_tx_dst *h_dsts, uint32_t ndst,
                     uint32_t slot_bytes, uint32_t flags, uint16_t *h_frame_len, uint8_t *h_status,
                     uint64_t *h_errors)
{
    if (n == 0) {
        if (h_errors)
            *h_errors = 0;
        return WC_OK;
    }
    if (flags & ~(uint32_t)WC_TX_ZERO_UDP_CKSUM) // (WC_TX_NO_STORE: the device call's)
        return WC_EINVAL;
    int rc = tx_build_args(h_base, h_off, h_desc, h_socks, ns, h_dsts, ndst, h_frame_len, h_status);
    if (rc)
        return rc;
    const bool zero_udp = flags & WC_TX_ZERO_UDP_CKSUM;
    // The check chain, and every frame that passes inside the region, before
    // any byte is written.
    uint64_t nb = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const HostFrame f = host_frame(h_desc, i, h_socks, ns, h_dsts, ndst, slot_bytes, zero_udp);
        if (f.x.status > WC_TX_SEALED_ZERO_UDP)
            continue;
        if (h_off[i] > h_bytes || f.x.flen > h_bytes - h_off[i])
            return WC_EINVAL;
        ++nb;
    }
    // The built frames' offsets, lengths and results, compacted for the seal's
    // batch.
    uint64_t *off = new (std::nothrow) uint64_t[nb + 1];
    uint16_t *vals = new (std::nothrow) uint16_t[3 * nb + 1];
    uint8_t *st = new (std::nothrow) uint8_t[nb + 1];
    if (!off || !vals || !st) {
        delete[] off;
        delete[] vals;
        delete[] st;
        return WC_ENOMEM;
    }
    uint16_t *len = vals, *udp = vals + nb, *iph = vals + 2 * nb;
    uint8_t *hb = (uint8_t *)h_base;
    uint64_t k = 0, errs = 0;
    for (uint64_t i = 0; i < n; ++i) {
        const HostFrame f = host_frame(h_desc, i, h_socks, ns, h_dsts, ndst, slot_bytes, zero_udp);
        const bool built = f.x.status <= WC_TX_SEALED_ZERO_UDP;
        h_status[i] = (uint8_t)f.x.status;
        h_frame_len[i] = (uint16_t)(built ? f.x.flen : 0u);
        errs += !built;
        if (!built)
            continue;
        // mk_ip4_hdr / mk_ip6_hdr, the UDP fields and mk_eth_hdr, both
        // checksum fields 0
        const wc::txb::Hdr h = wc::txb::headers(f.x, f.d, f.w, f.t, 0u, zero_udp, false);
        wc::txb::store_headers(HostMem{}, (uint64_t)(uintptr_t)(hb + h_off[i]), f.x.v4, h.h);
        off[k] = h_off[i];
        len[k] = (uint16_t)f.x.flen;
        ++k;
    }
    rc = WC_OK;
    if (nb) {
        rc = host_batch(h_base, h_bytes, off, len, nb, {{(uint8_t *)udp, (uint8_t *)iph, st}},
                        zero_udp ? kKindTxZero : kKindTx);
        // The two stores, as wc_tx_seal_host makes them: every frame here is one
        // the seal's chain accepts (its status is the build's), and its IHL
        // says the 20 bytes the build wrote.
        for (k = 0; rc == WC_OK && k < nb; ++k) {
            if (st[k] > WC_TX_SEALED_ZERO_UDP) {
                rc = WC_EINVAL; // (cannot happen: the headers above are the chain's)
                break;
            }
            tx_store_sums(hb + off[k], st[k], iph[k], udp[k]);
        }
    }
    if (rc == WC_OK && h_errors)
        *h_errors = errs;
    delete[] off;
    delete[] vals;
    delete[] st;
    return rc;
}

} // extern "C"
