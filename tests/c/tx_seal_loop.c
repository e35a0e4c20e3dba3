/*
 * tx_seal_loop.c -- the TX seal hook of INTEGRATION.md section 3, compiled and
 * driven the way the reference sends a w_iov_sq.
 *
 * The reference's w_tx walks the queue iov by iov and calls udp_tx on each
 * (/root/reference/lib/src/backend_netmap.c:348-358): udp_tx fills the IP
 * header (mk_ip4_hdr: ip4.c:153-186) and the UDP header and stores both
 * checksums into the frame (ip4.c:184-186, udp.c:209-213).  The hook here
 * builds every iov's headers WITHOUT touching the two checksum fields -- they
 * keep whatever the buffer held, here 0x0000, 0xFFFF or random bytes -- and
 * then makes ONE wc_tx_seal_host call per queue over the frames themselves
 * (buffer offset, 14 + IP length): no IP header is looked for on the CPU, no
 * result array comes back, no second store pass runs.  A zero-checksum
 * socket's queue passes WC_TX_ZERO_UDP_CKSUM.
 *
 * Every frame is then compared byte for byte (its whole 2048-B buffer) with
 * the same frame finished on the CPU by the oracle -- both fields zeroed,
 * oracle_ip_cksum / oracle_payload_cksum stored raw -- and every status must
 * be WC_TX_SEALED (WC_TX_SEALED_ZERO_UDP for the zero-checksum sockets).
 * Short queues are sealed a second time (the ring-full retry of
 * backend_netmap.c:353-356 needs no special handling): nothing may change.
 * The frames then go onto a "wire" and through wc_rx_verdict_host, the
 * reference's RX checks: each must be WC_RX_OK, or WC_RX_OK_NO_CKSUM where the
 * stored UDP field is 0.
 *
 * Sockets: IPv4, IPv4 with header options, IPv6, and a zero-checksum socket
 * of each family.  Queues of 1, 5, 300 and 5000 iovs; pass 0 on a registered
 * region (zero-copy launch, in-place streaming), pass 1 on a pageable one
 * (the pipeline).  The resident server is never asked.
 *
 *   tx_seal_loop
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "warpcore_gpu/wc_cksum.h"
#include "wc_oracle.h"

#define RING_SEED 0x9E3779B97F4A7C15ull
#include "ring.h"
#define MAX_Q 5000

enum { S_V4, S_V4_OPTS, S_V6, S_V4_ZERO, S_V6_ZERO, NSOCK };

struct sock { /* the w_sock fields udp_tx reads */
    int af6, opt_hl, zero_cksum;
    uint8_t laddr[16], raddr[16];
    uint16_t lport, rport;
};

/* what an unwritten checksum field may hold */
static void garbage16(uint8_t *p)
{
    const uint32_t k = rnd() % 3;
    p[0] = k == 0 ? 0x00 : k == 1 ? 0xFF : (uint8_t)rnd();
    p[1] = k == 0 ? 0x00 : k == 1 ? 0xFF : (uint8_t)rnd();
}

/* mk_eth_hdr + mk_ip4_hdr / mk_ip6_hdr + the UDP header (udp.c:189-207) around
 * `plen` payload bytes, the checksum fields left as garbage; returns the frame
 * length. */
static uint16_t build_headers(uint8_t *frame, const struct sock *s, uint32_t plen)
{
    uint8_t *ip = frame + 14;
    uint32_t hl;
    memset(frame, 0, 12);
    frame[0] = 0x02; /* locally administered MACs */
    frame[6] = 0x02;
    frame[5] = (uint8_t)rnd();
    frame[11] = (uint8_t)rnd();
    if (s->af6) {
        put16(frame + 12, 0x86DD);
        hl = 40;
        ip[0] = 0x60;
        ip[1] = (uint8_t)(rnd() & 0x0F); /* traffic class / flow label */
        ip[2] = (uint8_t)rnd();
        ip[3] = (uint8_t)rnd();
        put16(ip + 4, (uint16_t)(8 + plen)); /* payload length */
        ip[6] = 17;                          /* next header UDP */
        ip[7] = 0xff;                        /* hop limit */
        memcpy(ip + 8, s->laddr, 16);
        memcpy(ip + 24, s->raddr, 16);
    } else {
        put16(frame + 12, 0x0800);
        hl = 20 + (uint32_t)s->opt_hl;
        ip[0] = (uint8_t)(0x40 | (hl >> 2));
        ip[1] = (uint8_t)(rnd() & 0xFC);
        put16(ip + 2, (uint16_t)(hl + 8 + plen));
        ip[4] = (uint8_t)rnd(); /* id: random (ip4.c:167) */
        ip[5] = (uint8_t)rnd();
        ip[6] = 0x40; /* IP4_DF */
        ip[7] = 0x00;
        ip[8] = 0xff; /* ttl */
        ip[9] = 17;
        garbage16(ip + 10); /* ip->cksum: the seal's */
        memcpy(ip + 12, s->laddr, 4);
        memcpy(ip + 16, s->raddr, 4);
        for (uint32_t i = 20; i < hl; i++)
            ip[i] = i + 1 == hl ? 0x00 : 0x01; /* NOPs, then end of options */
    }
    uint8_t *udp = ip + hl;
    put16(udp, s->lport);
    put16(udp + 2, s->rport);
    put16(udp + 4, (uint16_t)(8 + plen));
    garbage16(udp + 6); /* udp->cksum: the seal's */
    return (uint16_t)(14 + hl + 8 + plen);
}

/* mk_ip4_hdr's and udp_tx's stores on the CPU (ip4.c:184-186, udp.c:209-213) */
static void oracle_finish(uint8_t *frame, const struct sock *s)
{
    uint8_t *ip = frame + 14;
    const uint32_t hl = s->af6 ? 40 : (uint32_t)(ip[0] & 15) * 4;
    const uint16_t ulen = (uint16_t)((ip[hl + 4] << 8) | ip[hl + 5]);
    memset(ip + hl + 6, 0, 2);
    if (!s->af6) {
        memset(ip + 10, 0, 2);
        const uint16_t c = oracle_ip_cksum(ip, (uint16_t)hl);
        memcpy(ip + 10, &c, 2);
    }
    if (!s->zero_cksum) {
        const uint16_t c = oracle_payload_cksum(ip, (uint16_t)(hl + ulen));
        memcpy(ip + hl + 6, &c, 2);
    }
}

#define FAIL(...) RING_FAIL("tx_seal_loop", __VA_ARGS__)

int main(void)
{
    static const uint32_t qlen[] = {1, 5, 300, 5000};
    const int nq = (int)(sizeof qlen / sizeof qlen[0]);
    const uint32_t nbufs = MAX_Q + 64;
    const uint64_t mem_size = (uint64_t)nbufs * BUF_SIZE;
    uint32_t wire_cap = 0;
    for (int i = 0; i < nq; i++)
        wire_cap += 2 * NSOCK * qlen[i];
    uint8_t *mem = aligned_alloc(4096, mem_size); /* w->mem */
    uint8_t *ref = malloc(mem_size);              /* the same frames, finished by the oracle */
    uint32_t *free_idx = malloc(nbufs * sizeof *free_idx);
    uint64_t *off = malloc(MAX_Q * sizeof *off);
    uint16_t *len = malloc(MAX_Q * sizeof *len);
    uint8_t *status = malloc(MAX_Q), *status2 = malloc(MAX_Q);
    uint8_t *wire = aligned_alloc(4096, (uint64_t)wire_cap * BUF_SIZE);
    uint64_t *woff = malloc(wire_cap * sizeof *woff);
    uint16_t *wlen = malloc(wire_cap * sizeof *wlen);
    int *wsock = malloc(wire_cap * sizeof *wsock);
    uint8_t *verdict = malloc(wire_cap);
    if (!mem || !ref || !free_idx || !off || !len || !status || !status2 || !wire || !woff ||
        !wlen || !wsock || !verdict)
        FAIL("alloc");
    for (uint64_t i = 0; i < mem_size; i++) /* buffers are never clean */
        mem[i] = (uint8_t)rnd();
    for (uint32_t i = 0; i < nbufs; i++)
        free_idx[i] = i;

    struct sock socks[NSOCK];
    for (int k = 0; k < NSOCK; k++) {
        struct sock *s = &socks[k];
        s->af6 = k == S_V6 || k == S_V6_ZERO;
        s->opt_hl = k == S_V4_OPTS ? 4 * (1 + (int)(rnd() % 10)) : 0;
        s->zero_cksum = k == S_V4_ZERO || k == S_V6_ZERO;
        for (int i = 0; i < 16; i++) {
            s->laddr[i] = (uint8_t)rnd();
            s->raddr[i] = (uint8_t)rnd();
        }
        s->lport = (uint16_t)rnd();
        s->rport = (uint16_t)rnd();
    }

    uint64_t served0 = 0, fb0 = 0, served = 0, fb = 0;
    wc_server_stats(&served0, &fb0, NULL);
    uint32_t wn = 0;
    uint64_t calls = 0, reseals = 0;
    for (int pass = 0; pass < 2; pass++) {
        /* pass 0: w->mem registered; pass 1 pageable */
        if (pass == 0 && wc_host_register(mem, mem_size) != WC_OK)
            FAIL("wc_host_register");
        if (pass == 1 && wc_host_unregister(mem) != WC_OK)
            FAIL("wc_host_unregister");
        for (int qi = 0; qi < nq; qi++)
            for (int k = 0; k < NSOCK; k++) {
                const struct sock *s = &socks[k];
                const uint32_t n = qlen[qi];
                const uint32_t hl = s->af6 ? 40 : 20 + (uint32_t)s->opt_hl;
                /* w_alloc: buffers in scrambled order */
                ring_shuffle(free_idx, sizeof *free_idx, nbufs);
                /* the application's payloads, then udp_tx's headers: the
                 * queue as (buffer offset, frame length) */
                for (uint32_t i = 0; i < n; i++) {
                    uint8_t *frame = mem + (uint64_t)free_idx[i] * BUF_SIZE;
                    const uint32_t room = BUF_SIZE - 14 - hl - 8;
                    const uint32_t plen = rnd() % 5 == 0 ? rnd() % 16 : rnd() % (room + 1);
                    for (uint32_t b = 0; b < plen; b++)
                        frame[14 + hl + 8 + b] = (uint8_t)rnd();
                    off[i] = (uint64_t)free_idx[i] * BUF_SIZE;
                    len[i] = build_headers(frame, s, plen);
                }
                memcpy(ref, mem, mem_size);
                for (uint32_t i = 0; i < n; i++)
                    oracle_finish(ref + off[i], s);
                /* ONE call for the queue */
                const uint32_t flags = s->zero_cksum ? WC_TX_ZERO_UDP_CKSUM : 0;
                uint64_t errs = ~0ull;
                int rc = wc_tx_seal_host(mem, mem_size, off, len, n, flags, status, &errs);
                if (rc != WC_OK)
                    FAIL("wc_tx_seal_host: %s (%d)", wc_strerror(rc), rc);
                ++calls;
                if (errs)
                    FAIL("sock %d queue %u: %llu error frames", k, n, (unsigned long long)errs);
                const int want = s->zero_cksum ? WC_TX_SEALED_ZERO_UDP : WC_TX_SEALED;
                for (uint32_t i = 0; i < n; i++)
                    if (status[i] != want)
                        FAIL("sock %d queue %u iov %u: status %d, expected %d", k, n, i, status[i],
                             want);
                if (memcmp(mem, ref, mem_size)) {
                    uint64_t at = 0;
                    while (mem[at] == ref[at])
                        ++at;
                    FAIL("sock %d queue %u pass %d: byte %llu (buffer %llu + %llu) is %02x, the "
                         "oracle's frame has %02x", k, n, pass, (unsigned long long)at,
                         (unsigned long long)(at / BUF_SIZE), (unsigned long long)(at % BUF_SIZE),
                         mem[at], ref[at]);
                }
                if (n <= 300) { /* the ring-full retry: sealing again changes nothing */
                    rc = wc_tx_seal_host(mem, mem_size, off, len, n, flags, status2, &errs);
                    if (rc != WC_OK || errs || memcmp(status, status2, n) ||
                        memcmp(mem, ref, mem_size))
                        FAIL("sock %d queue %u: the second seal changed something (rc %d)", k, n,
                             rc);
                    ++reseals;
                }
                /* w_nic_tx: onto the wire */
                for (uint32_t i = 0; i < n; i++, wn++) {
                    memcpy(wire + (uint64_t)wn * BUF_SIZE, mem + off[i], len[i]);
                    woff[wn] = (uint64_t)wn * BUF_SIZE;
                    wlen[wn] = len[i];
                    wsock[wn] = k;
                }
            }
    }
    wc_server_stats(&served, &fb, NULL);
    if (served != served0 || fb != fb0)
        FAIL("the resident server was asked (%llu served, %llu fallbacks)",
             (unsigned long long)(served - served0), (unsigned long long)(fb - fb0));
    if (wn != wire_cap)
        FAIL("wire holds %u frames of %u", wn, wire_cap);
    /* the receiver: the reference's RX checks on every frame */
    uint64_t drops = 0, no_cksum = 0;
    if (wc_host_register(wire, (uint64_t)wn * BUF_SIZE) != WC_OK)
        FAIL("wc_host_register wire");
    const int rc = wc_rx_verdict_host(wire, (uint64_t)wn * BUF_SIZE, woff, wlen, wn, verdict, &drops);
    wc_host_unregister(wire);
    if (rc != WC_OK)
        FAIL("wc_rx_verdict_host: %s (%d)", wc_strerror(rc), rc);
    for (uint32_t i = 0; i < wn; i++) {
        const uint8_t *fr = wire + woff[i];
        const uint32_t hl = socks[wsock[i]].af6 ? 40 : (uint32_t)(fr[14] & 15) * 4;
        const int field0 = fr[14 + hl + 6] == 0 && fr[14 + hl + 7] == 0;
        const int want = field0 ? WC_RX_OK_NO_CKSUM : WC_RX_OK;
        if (socks[wsock[i]].zero_cksum && !field0)
            FAIL("wire frame %u: a zero-checksum socket's UDP field is not 0", i);
        if (verdict[i] != want || oracle_rx_verdict(fr, wlen[i]) != want)
            FAIL("wire frame %u (sock %d): gpu %d oracle %d expected %d", i, wsock[i], verdict[i],
                 oracle_rx_verdict(fr, wlen[i]), want);
        no_cksum += verdict[i] == WC_RX_OK_NO_CKSUM;
    }
    if (drops)
        FAIL("%llu frames dropped", (unsigned long long)drops);
    wc_gpu_fini();
    printf("tx_seal_loop: ok (%u iovs sealed in %llu calls, %llu queues sealed twice unchanged, "
           "every frame byte-identical to the oracle's and accepted by the RX checks, %llu without "
           "UDP checksum)\n", wn, (unsigned long long)calls, (unsigned long long)reseals,
           (unsigned long long)no_cksum);
    return 0;
}
