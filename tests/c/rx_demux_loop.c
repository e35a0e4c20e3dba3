/*
 * rx_demux_loop.c -- the RX demultiplex hook of INTEGRATION.md section 3,
 * compiled and driven the way the reference drains a netmap RX ring
 * (w_nic_rx, /root/reference/lib/src/backend_netmap.c:379-391) and queues
 * what it accepts on its sockets (udp_rx, udp.c:141-156, 174).
 *
 * An engine with a handful of bound and connected sockets, IPv4 and IPv6.
 * Per pass the hook builds the socket table (as after a w_bind / w_connect),
 * gathers the ring's offsets and lengths, calls wc_rx_demux_host ONCE and
 * links socket s's queue from the run h_list[h_start[s] .. h_start[s + 1]):
 * no header line of a delivered frame is touched and nothing is hashed on the
 * host.  The check: a plain per-frame loop over the same ring -- the oracle's
 * verdict, local and remote from the frame's own bytes, the connected tuple
 * and then the bound one looked up by comparing every socket in turn,
 * appended in ring order -- must give the same queues, entry for entry, and
 * the same unbound frames; wc_rx_socktab_lookup must answer like that loop;
 * and verdicts, records and drops must be wc_rx_deliver_host's.  Pass 0 runs
 * on the registered region, pass 1 on pageable memory with the sockets
 * reshuffled.
 *
 *   rx_demux_loop [slots]
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "warpcore_gpu/wc_cksum.h"
#include "wc_oracle.h"

#define RING_SEED 0xD1B54A32D192ED03ull
#include "ring.h"
#define NSOCKS 12

/* The engine's sockets: bound and connected ones sharing a local pair, an
 * IPv4 and an IPv6 socket alike in four address bytes and the port, one port
 * on two addresses; garbage in the bytes the library ignores. */
static void make_socks(struct wc_rx_sock *s)
{
    static const uint8_t a[2][4] = {{10, 0, 0, 1}, {10, 0, 0, 2}}, peer[4] = {192, 168, 1, 9};
    memset(s, 0xA5, NSOCKS * sizeof *s);
    for (int i = 0; i < NSOCKS; i++) {
        const int v6 = i >= 6, conn = i % 3 == 1;
        s[i].af = v6 ? 6 : 4;
        s[i].connected = (uint8_t)conn;
        memcpy(s[i].laddr, a[(i / 3) & 1], 4);
        if (v6)
            memset(s[i].laddr + 4, 0x11, 12);
        put16((uint8_t *)&s[i].lport, (uint16_t)(4433 + (i % 3 == 2)));
        if (conn) {
            memcpy(s[i].raddr, peer, 4);
            if (v6)
                memset(s[i].raddr + 4, 0x22, 12);
            put16((uint8_t *)&s[i].rport, 7000);
        }
    }
}

enum { C_TO_SOCK, C_TO_SOCK_OPTS, C_STRAY, C_NO_CKSUM, C_BAD_UDP, C_ICMP, C_ARP, C_TRUNC, NCASES };

/* A frame of case k; C_TO_SOCK*: to socket `to`, from its remote if it is
 * connected (else from a random one -- or, one time in four, from the remote
 * of its connected sibling at another port). */
static uint16_t make_frame(uint8_t *f, int k, const struct wc_rx_sock *socks, int to)
{
    const struct wc_rx_sock *s = &socks[to];
    const int v6 = (k == C_TO_SOCK || k == C_TO_SOCK_OPTS || k == C_NO_CKSUM) ? s->af == 6
                                                                             : (int)(rnd() & 1);
    const uint32_t hl = v6 ? 40 : (k == C_TO_SOCK_OPTS ? 24 + 4 * (rnd() % 10) : 20);
    const uint32_t pay = rnd() % 1200;
    const uint32_t ip_len = hl + 8 + pay;
    for (uint32_t i = 0; i < 14 + ip_len; i++)
        f[i] = (uint8_t)rnd();
    put16(f + 12, k == C_ARP ? 0x0806 : v6 ? 0x86DD : 0x0800);
    uint8_t *ip = f + 14, *udp = ip + hl;
    uint8_t *src = ip + (v6 ? 8 : 12), *dst = ip + (v6 ? 24 : 16);
    if (k == C_TO_SOCK || k == C_TO_SOCK_OPTS || k == C_NO_CKSUM) {
        const unsigned alen = v6 ? 16 : 4;
        memcpy(dst, s->laddr, alen);
        memcpy(udp + 2, &s->lport, 2);
        if (s->connected) {
            memcpy(src, s->raddr, alen);
            memcpy(udp, &s->rport, 2);
        } else if (rnd() % 4 == 0) {
            memcpy(src, socks[1].raddr, 4); /* the peer's first bytes, another port */
            put16(udp, 7001);
        }
    }
    if (v6) {
        ip[0] = (uint8_t)(0x60 | (ip[0] & 0x0F));
        put16(ip + 4, (uint16_t)(ip_len - 40));
        ip[6] = k == C_ICMP ? 58 : 17;
    } else {
        ip[0] = (uint8_t)(0x40 | (hl / 4));
        put16(ip + 2, (uint16_t)ip_len);
        ip[6] = 0x40;
        ip[7] = 0;
        ip[9] = k == C_ICMP ? 1 : 17;
        ip[10] = ip[11] = 0;
        const uint16_t hc = oracle_ip_cksum(ip, (uint16_t)hl);
        memcpy(ip + 10, &hc, 2);
    }
    put16(udp + 4, (uint16_t)(8 + pay));
    udp[6] = udp[7] = 0;
    if (k != C_NO_CKSUM) {
        uint16_t uc = oracle_payload_cksum(ip, (uint16_t)(hl + 8 + pay));
        if (uc == 0)
            uc = 0xFFFF;
        memcpy(udp + 6, &uc, 2);
    }
    if (k == C_BAD_UDP)
        udp[8 + pay - 1] ^= 0x10, udp[3] ^= (uint8_t)(pay == 0);
    if (k == C_TRUNC)
        return (uint16_t)(14 + hl + 4);
    return (uint16_t)(14 + ip_len);
}

/* w_get_sock by comparing every socket in turn (warpcore.c:644-677): the
 * connected tuple, then the bound one (udp.c:143-146). */
static int plain_lookup(const struct wc_rx_sock *socks, uint8_t af, const uint8_t *laddr,
                        uint16_t lport, const uint8_t *raddr, uint16_t rport)
{
    const unsigned alen = af == 4 ? 4 : 16;
    for (int conn = 1; conn >= 0; conn--)
        for (int i = 0; i < NSOCKS; i++) {
            const struct wc_rx_sock *s = &socks[i];
            if (s->af != af || s->connected != conn || s->lport != lport ||
                memcmp(s->laddr, laddr, alen))
                continue;
            if (conn && (s->rport != rport || memcmp(s->raddr, raddr, alen)))
                continue;
            return i;
        }
    return WC_RX_SOCK_UNBOUND;
}

#define FAIL(...) RING_FAIL("rx_demux_loop", __VA_ARGS__)

int main(int argc, char **argv)
{
    const uint32_t nslots = argc > 1 ? (uint32_t)atoi(argv[1]) : 6000;
    const uint64_t mem_size = (uint64_t)nslots * BUF_SIZE;
    uint8_t *mem = aligned_alloc(4096, mem_size);
    struct nm_slot *slot = calloc(nslots, sizeof *slot);
    uint64_t *off = malloc(nslots * sizeof *off), start[256];
    uint16_t *flen = malloc(nslots * sizeof *flen);
    uint8_t *verdict = malloc(nslots), *verdict2 = malloc(nslots), *sock = malloc(nslots);
    struct wc_rx_record *rec = malloc(nslots * sizeof *rec), *rec2 = malloc(nslots * sizeof *rec);
    uint32_t *list = malloc(nslots * sizeof *list);
    /* the plain loop's queues: NSOCKS sockets and the unbound frames */
    uint32_t *queue[NSOCKS + 1], qlen[NSOCKS + 1];
    void *tab = malloc(wc_rx_socktab_bytes(NSOCKS));
    struct wc_rx_sock socks[NSOCKS];
    if (!mem || !slot || !off || !flen || !verdict || !verdict2 || !sock || !rec || !rec2 ||
        !list || !tab)
        FAIL("alloc");
    for (int q = 0; q <= NSOCKS; q++)
        if (!(queue[q] = malloc(nslots * sizeof **queue)))
            FAIL("alloc");
    for (uint32_t i = 0; i < nslots; i++)
        slot[i].buf_idx = i;
    ring_shuffle(&slot[0].buf_idx, sizeof *slot, nslots);
    make_socks(socks);
    uint64_t queued = 0, unbound = 0;
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 0 && wc_host_register(mem, mem_size) != WC_OK)
            FAIL("wc_host_register");
        if (pass == 1) {
            if (wc_host_unregister(mem) != WC_OK)
                FAIL("wc_host_unregister");
            for (int i = NSOCKS - 1; i > 0; i--) { /* the sockets in another order */
                const int j = (int)(rnd() % (uint32_t)(i + 1));
                const struct wc_rx_sock t = socks[i];
                socks[i] = socks[j];
                socks[j] = t;
            }
        }
        if (wc_rx_socktab_build(socks, NSOCKS, tab) != WC_OK)
            FAIL("wc_rx_socktab_build");
        for (uint32_t s = 0; s < nslots; s++) {
            slot[s].len = make_frame(mem + (uint64_t)slot[s].buf_idx * BUF_SIZE,
                                     (int)(rnd() % NCASES), socks, (int)(rnd() % NSOCKS));
            off[s] = (uint64_t)slot[s].buf_idx * BUF_SIZE;
            flen[s] = slot[s].len;
        }
        memset(list, 0xEE, nslots * sizeof *list);
        memset(sock, 0xEE, nslots);
        uint64_t drops = ~0ull, drops2 = ~0ull;
        int rc = wc_rx_demux_host(mem, mem_size, off, flen, nslots, tab, NSOCKS, verdict, rec, sock,
                                  list, start, &drops);
        if (rc != WC_OK)
            FAIL("wc_rx_demux_host: %s (%d)", wc_strerror(rc), rc);
        rc = wc_rx_deliver_host(mem, mem_size, off, flen, nslots, verdict2, rec2, NULL, NULL,
                                &drops2);
        if (rc != WC_OK)
            FAIL("wc_rx_deliver_host: %s (%d)", wc_strerror(rc), rc);
        if (memcmp(verdict, verdict2, nslots) || memcmp(rec, rec2, nslots * sizeof *rec) ||
            drops != drops2)
            FAIL("verdicts, records or drops differ from wc_rx_deliver_host's");
        /* the plain loop: udp.c:141-156 and 174, frame by frame in ring order */
        memset(qlen, 0, sizeof qlen);
        for (uint32_t s = 0; s < nslots; s++) {
            const uint8_t *buf = mem + off[s], *ip = buf + 14;
            const int v = oracle_rx_verdict(buf, flen[s]);
            if (v != verdict[s])
                FAIL("slot %u: verdict %d, oracle %d", s, verdict[s], v);
            if (v != WC_RX_OK && v != WC_RX_OK_NO_CKSUM) {
                if (sock[s] != WC_RX_SOCK_NONE)
                    FAIL("slot %u is not delivered but has socket %u", s, sock[s]);
                continue;
            }
            const int v4 = (ip[0] >> 4) == 4;
            const uint8_t *udp = ip + (v4 ? (ip[0] & 0x0F) * 4 : 40);
            uint16_t sport, dport;
            memcpy(&sport, udp, 2);
            memcpy(&dport, udp + 2, 2);
            const uint8_t *src = ip + (v4 ? 12 : 8), *dst = ip + (v4 ? 16 : 24);
            const int ws = plain_lookup(socks, v4 ? 4 : 6, dst, dport, src, sport);
            if (sock[s] != ws)
                FAIL("slot %u: socket %u, the plain loop's %d", s, sock[s], ws);
            if (wc_rx_socktab_lookup(tab, v4 ? 4 : 6, dst, dport, src, sport) != ws)
                FAIL("slot %u: wc_rx_socktab_lookup disagrees with the plain loop", s);
            const int q = ws == WC_RX_SOCK_UNBOUND ? NSOCKS : ws;
            queue[q][qlen[q]++] = s; /* sq_insert_tail */
        }
        /* the hook's queues: socket s's run of the list, as it stands */
        for (int q = 0; q <= NSOCKS; q++) {
            const uint64_t lo = q == NSOCKS ? start[254] : start[q];
            const uint64_t hi = q == NSOCKS ? start[255] : start[q + 1];
            if (hi - lo != qlen[q])
                FAIL("queue %d: %llu frames, the plain loop queued %u", q,
                     (unsigned long long)(hi - lo), qlen[q]);
            if (memcmp(list + lo, queue[q], qlen[q] * sizeof *list))
                FAIL("queue %d differs from the plain loop's", q);
            if (q < NSOCKS)
                queued += qlen[q];
            else
                unbound += qlen[q];
        }
        for (int s = NSOCKS; s < 254; s++)
            if (start[s] != start[254])
                FAIL("start[%d] is not the unbound run's start", s);
        for (uint64_t q = start[255]; q < nslots; q++)
            if (list[q] != 0xEEEEEEEEu)
                FAIL("list entry %llu past the total was written", (unsigned long long)q);
    }
    wc_gpu_fini();
    printf("rx_demux_loop: ok (%u slots, 2 passes: %llu frames queued on %d sockets, %llu "
           "unbound)\n",
           nslots, (unsigned long long)queued, NSOCKS, (unsigned long long)unbound);
    return 0;
}
