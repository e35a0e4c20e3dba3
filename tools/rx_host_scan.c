/*
 * rx_host_scan.c -- what RX delivery replaces on the host, timed on one core
 * (tools/rx_deliver.py builds and runs it with the C oracle's flags,
 * oracle/Makefile: -Ofast -march=native): after wc_rx_verdict_*, the
 * integrator scans all n verdict bytes for the accepted frames and re-reads
 * each one's Ethernet / IP / UDP headers to fill the w_iov as udp_rx does
 * (udp.c:101-142, 163-165).
 *
 * The ring is the mixed ring's shape: n frames, one per 2048-B slot, 2:1
 * IPv4 / IPv6 UDP headers (only the header bytes matter here; they are
 * written, the payload is not), every `arp`-th verdict NOT_IP, the rest OK.
 * Prints the best and median of `reps` passes of the scan alone and of scan +
 * re-parse.
 *
 *   rx_host_scan [n = 2^21] [arp_every = 0] [reps = 7]
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#define SLOT 2048

struct iov {
    const uint8_t *base, *buf;
    uint16_t len, port, lport;
    uint8_t af, flags, ttl;
    uint8_t addr[16], local[16];
};

static double now(void)
{
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double)t.tv_sec + 1e-9 * (double)t.tv_nsec;
}

static inline void udp_rx_fill(const uint8_t *buf, struct iov *i)
{
    const uint8_t *ip = buf + 14;
    uint16_t hl, ip_plen;
    if ((ip[0] >> 4) == 4) {
        hl = (uint16_t)((ip[0] & 0x0F) * 4);
        ip_plen = (uint16_t)(((ip[2] << 8) | ip[3]) - hl);
        i->af = 4;
        memcpy(i->addr, ip + 12, 4);
        memcpy(i->local, ip + 16, 4);
        i->flags = ip[1];
        i->ttl = ip[8];
    } else {
        uint32_t vtcecnfl;
        memcpy(&vtcecnfl, ip, 4);
        hl = 40;
        ip_plen = (uint16_t)((ip[4] << 8) | ip[5]);
        i->af = 6;
        memcpy(i->addr, ip + 8, 16);
        memcpy(i->local, ip + 24, 16);
        i->flags = (uint8_t)(((vtcecnfl & 0x0000f000) >> 12) | ((vtcecnfl & 0x0000000f) << 4));
        i->ttl = ip[7];
    }
    const uint8_t *udp = ip + hl;
    const uint16_t ul = (uint16_t)((udp[4] << 8) | udp[5]);
    i->len = (uint16_t)((ul < ip_plen ? ul : ip_plen) - 8);
    memcpy(&i->port, udp, 2);
    memcpy(&i->lport, udp + 2, 2);
    i->base = buf;
    i->buf = udp + 8;
}

static int cmp(const void *a, const void *b)
{
    const double x = *(const double *)a, y = *(const double *)b;
    return (x > y) - (x < y);
}

int main(int argc, char **argv)
{
    const uint64_t n = argc > 1 ? strtoull(argv[1], 0, 0) : 1ull << 21;
    const uint64_t arp = argc > 2 ? strtoull(argv[2], 0, 0) : 0;
    const int reps = argc > 3 ? atoi(argv[3]) : 7;
    uint8_t *mem = malloc(n * SLOT);
    uint8_t *verdict = malloc(n);
    uint32_t *list = malloc(n * sizeof *list);
    double *t_scan = malloc(reps * sizeof(double)), *t_all = malloc(reps * sizeof(double));
    if (!mem || !verdict || !list || !t_scan || !t_all)
        return 1;
    uint64_t x = 0x9E3779B97F4A7C15ull;
    for (uint64_t i = 0; i < n; i++) {
        uint8_t *f = mem + i * SLOT;
        for (int k = 0; k < 64; k += 8) {
            x ^= x << 13, x ^= x >> 7, x ^= x << 17;
            memcpy(f + k, &x, 8);
        }
        const int v6 = i % 3 == 0;
        f[12] = v6 ? 0x86 : 0x08;
        f[13] = v6 ? 0xDD : 0x00;
        f[14] = v6 ? 0x60 : 0x45;
        verdict[i] = arp && i % arp == 0 ? 8 : 0;
    }
    volatile uint64_t sink = 0;
    for (int r = 0; r < reps; r++) {
        double t0 = now();
        uint64_t cnt = 0;
        for (uint64_t i = 0; i < n; i++)
            if (verdict[i] <= 1)
                list[cnt++] = (uint32_t)i;
        t_scan[r] = now() - t0;
        uint64_t acc = 0;
        for (uint64_t k = 0; k < cnt; k++) {
            struct iov v;
            udp_rx_fill(mem + (uint64_t)list[k] * SLOT, &v);
            acc += v.len + v.port + v.lport + v.af + v.flags + v.ttl + v.addr[0] + v.local[3] +
                   (uint64_t)(v.buf - v.base);
        }
        t_all[r] = now() - t0;
        sink += acc + cnt;
    }
    qsort(t_scan, reps, sizeof(double), cmp);
    qsort(t_all, reps, sizeof(double), cmp);
    printf("rx_host_scan: n %llu, arp_every %llu, one core: verdict scan best %.1f us median %.1f "
           "us; scan + header re-parse best %.1f us median %.1f us (%d passes)\n",
           (unsigned long long)n, (unsigned long long)arp, 1e6 * t_scan[0], 1e6 * t_scan[reps / 2],
           1e6 * t_all[0], 1e6 * t_all[reps / 2], reps);
    return (int)(sink & 0);
}
