/*
 * rx_host_demux.c -- what wc_rx_demux replaces on the host, timed on one core
 * (tools/rx_demux.py --host-demux builds and runs it with the C oracle's
 * flags, oracle/Makefile: -Ofast -march=native): after wc_rx_deliver_*, the
 * integrator walks the delivered list, reads each frame's two addresses
 * through its record's src_off / dst_off, looks the socket up
 * (wc_rx_socktab_lookup: the connected tuple, then the bound one) and appends
 * the frame to that socket's queue (udp.c:141-156, 174).
 *
 * The ring is the mixed ring's shape: n frames, one per 2048-B slot, 2:1
 * IPv4 / IPv6 (only the header bytes matter here; they are written, the
 * payload is not), every frame delivered and aimed at one of `ns` sockets, so
 * every lookup ends on a full compare.  Prints the best and median of `reps`
 * passes.
 *
 *   rx_host_demux [n = 2^21] [ns = 16] [reps = 7]
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#include "warpcore_gpu/wc_cksum.h"

#define SLOT 2048

static double now(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

static int cmp(const void *a, const void *b)
{
    const double x = *(const double *)a, y = *(const double *)b;
    return (x > y) - (x < y);
}

int main(int argc, char **argv)
{
    const uint64_t n = argc > 1 ? strtoull(argv[1], 0, 0) : 1ull << 21;
    const uint32_t ns = argc > 2 ? (uint32_t)atoi(argv[2]) : 16;
    const int reps = argc > 3 ? atoi(argv[3]) : 7;
    if (ns < 1 || ns > WC_RX_DEMUX_MAX_SOCKS)
        return 2;
    uint8_t *mem = malloc(n * SLOT);
    struct wc_rx_record *rec = calloc(n, sizeof *rec);
    uint32_t *list = malloc(n * sizeof *list);
    uint32_t *queue = calloc(n, sizeof *queue); /* queue[i]: the frame queued behind frame i */
    uint64_t *qlen = calloc(256, sizeof *qlen), *qat = calloc(256, sizeof *qat);
    struct wc_rx_sock *socks = calloc(ns, sizeof *socks);
    void *tab = malloc(wc_rx_socktab_bytes(ns));
    double *t = malloc(reps * sizeof(double));
    if (!mem || !rec || !list || !queue || !qlen || !qat || !socks || !tab || !t)
        return 1;
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (uint32_t j = 0; j < ns; j++) { /* every third IPv6, every second connected */
        socks[j].af = j % 3 == 2 ? 6 : 4;
        socks[j].connected = j & 1;
        for (int k = 0; k < 16; k++) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            socks[j].laddr[k] = (uint8_t)x;
            socks[j].raddr[k] = (uint8_t)(x >> 8);
        }
        socks[j].lport = (uint16_t)(1024 + j);
        socks[j].rport = (uint16_t)(40000 + j);
    }
    if (wc_rx_socktab_build(socks, ns, tab) != WC_OK)
        return 3;
    for (uint64_t i = 0; i < n; i++) {
        uint8_t *f = mem + i * SLOT;
        for (int k = 0; k < 64; k += 8) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            memcpy(f + k, &x, 8);
        }
        uint32_t j = (uint32_t)((i * 2654435761ull) >> 8) % ns;
        const int v6 = ns >= 3 && i % 3 == 0; /* (fewer sockets: all IPv4) */
        while ((socks[j].af == 6) != v6)
            j = (j + 1) % ns;
        const unsigned alen = v6 ? 16 : 4;
        struct wc_rx_record *r = &rec[i];
        r->af = v6 ? 6 : 4;
        r->hl = v6 ? 40 : 20;
        r->src_off = (uint16_t)(14 + (v6 ? 8 : 12));
        r->dst_off = (uint16_t)(14 + (v6 ? 24 : 16));
        r->dport = socks[j].lport;
        r->sport = socks[j].rport;
        memcpy(f + r->dst_off, socks[j].laddr, alen);
        memcpy(f + r->src_off, socks[j].raddr, alen);
        list[i] = (uint32_t)i;
    }
    volatile uint64_t sink = 0;
    for (int rep = 0; rep < reps; rep++) {
        memset(qlen, 0, 256 * sizeof *qlen);
        const double t0 = now();
        for (uint64_t k = 0; k < n; k++) {
            const uint32_t i = list[k];
            const struct wc_rx_record *r = &rec[i];
            const uint8_t *f = mem + (uint64_t)i * SLOT;
            const uint8_t s = wc_rx_socktab_lookup(tab, r->af, f + r->dst_off, r->dport,
                                                   f + r->src_off, r->sport);
            /* sq_insert_tail: the frame behind the socket's last one */
            if (qlen[s]++)
                queue[qat[s]] = i;
            qat[s] = i;
        }
        t[rep] = now() - t0;
        sink += queue[n / 2] + qlen[0] + qlen[255] + qat[0];
    }
    qsort(t, reps, sizeof(double), cmp);
    printf("rx_host_demux: n %llu, %u sockets, one core: list walk + address reads + lookup + "
           "append best %.1f us median %.1f us (%d passes; %llu frames unbound)\n",
           (unsigned long long)n, ns, 1e6 * t[0], 1e6 * t[reps / 2], reps,
           (unsigned long long)qlen[255]);
    return (int)(sink & 0);
}
