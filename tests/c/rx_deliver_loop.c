/*
 * rx_deliver_loop.c -- the RX delivery hook of INTEGRATION.md section 3,
 * compiled and driven the way the reference drains a netmap RX ring
 * (w_nic_rx, /root/reference/lib/src/backend_netmap.c:379-391).
 *
 * A ring of slots {buf_idx, len} over buffers in one region (w->mem), in a
 * scrambled buf_idx order.  Per pass the hook gathers the slots' offsets and
 * lengths, calls wc_rx_deliver_host ONCE, and then touches no header of a
 * delivered frame: it walks only h_list, fills a w_iov-shaped struct from
 * h_rec[i] (the two addresses copied from src_off / dst_off), and hands it
 * to a stand-in for the socket lookup.  The check: the same struct filled
 * the way udp_rx does (udp.c:101-142, 163-165), by parsing the frame on the
 * CPU, must be equal byte for byte; h_list must be exactly the frames built
 * to be accepted, in ring order; and the WC_RX_MASK_HOST list, made by a
 * host pass over the verdict bytes (what wc_rx_select computes on a device),
 * must be exactly the ARP / ICMP frames.  Pass 0 runs on the registered
 * region, pass 1 on pageable memory.
 *
 *   rx_deliver_loop [slots]
 */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "warpcore_gpu/wc_cksum.h"
#include "wc_oracle.h"

#define RING_SEED 0x9E3779B97F4A7C15ull
#include "ring.h"

/* the w_iov fields udp_rx fills (warpcore.h), and the local address it looks
 * the socket up by */
struct iov {
    const uint8_t *base, *buf;
    uint16_t len;
    uint16_t port;  /* wv_port: udp->sport as stored */
    uint16_t lport; /* local.port: udp->dport as stored */
    uint8_t af, flags, ttl;
    uint8_t addr[16];  /* wv_ip4 / wv_ip6 */
    uint8_t local[16]; /* local.addr */
};

enum { C_OK4, C_OK4_OPTS, C_OK6, C_NO_CKSUM, C_ULEN_SHORT, C_BAD_UDP, C_BAD_UDP_OPTS, C_BAD_IP,
       C_FRAGMENT, C_ICMP4, C_ICMP6, C_ARP, C_TRUNC, NCASES };

static int accepted(int k) { return k <= C_ULEN_SHORT; }
static int hosts(int k) { return k == C_ICMP4 || k == C_ICMP6 || k == C_ARP; }

static uint16_t make_frame(uint8_t *f, int k)
{
    const int v6 = k == C_OK6 || k == C_ICMP6;
    const int opts = k == C_OK4_OPTS || k == C_BAD_UDP_OPTS;
    const uint32_t hl = v6 ? 40 : (opts ? 24 + 4 * (rnd() % 10) : 20); /* IHL 6..15 */
    const uint32_t pay = rnd() % 1400;
    const uint32_t ip_len = hl + 8 + pay;
    for (uint32_t i = 0; i < 14 + ip_len; i++)
        f[i] = (uint8_t)rnd();
    put16(f + 12, k == C_ARP ? 0x0806 : v6 ? 0x86DD : 0x0800);
    uint8_t *ip = f + 14, *udp = ip + hl;
    uint16_t ulen = (uint16_t)(8 + pay);
    if (k == C_ULEN_SHORT)
        ulen = (uint16_t)(8 + pay / 2);
    if (v6) {
        ip[0] = (uint8_t)(0x60 | (ip[0] & 0x0F)); /* a random traffic class */
        put16(ip + 4, (uint16_t)(ip_len - 40));
        ip[6] = k == C_ICMP6 ? 58 : 17;
    } else {
        ip[0] = (uint8_t)(0x40 | (hl / 4));
        put16(ip + 2, (uint16_t)ip_len);
        ip[6] = 0x40;
        ip[7] = 0;
        if (k == C_FRAGMENT)
            ip[6] = 0, ip[7] = (uint8_t)(1 + rnd() % 200);
        ip[9] = k == C_ICMP4 ? 1 : 17;
        ip[10] = ip[11] = 0;
        const uint16_t hc = oracle_ip_cksum(ip, (uint16_t)hl);
        memcpy(ip + 10, &hc, 2);
    }
    put16(udp + 4, ulen);
    udp[6] = udp[7] = 0;
    if (k != C_NO_CKSUM) {
        uint16_t uc = oracle_payload_cksum(ip, (uint16_t)(hl + ulen));
        if (uc == 0)
            uc = 0xFFFF;
        memcpy(udp + 6, &uc, 2);
    }
    if (k == C_BAD_UDP || k == C_BAD_UDP_OPTS)
        udp[2] += 1;
    if (k == C_BAD_IP)
        ip[8] += 1;
    if (k == C_TRUNC)
        return (uint16_t)(14 + hl + 4);
    return (uint16_t)(14 + ip_len);
}

/* udp_rx (udp.c:94-142, 163-165) on a frame the checks have passed */
static void udp_rx_fill(const uint8_t *buf, struct iov *i)
{
    memset(i, 0, sizeof *i);
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
    const uint16_t udp_len = ul < ip_plen ? ul : ip_plen;
    i->len = (uint16_t)(udp_len - 8);
    memcpy(&i->port, udp, 2);
    memcpy(&i->lport, udp + 2, 2);
    i->base = buf;
    i->buf = udp + 8;
}

/* the same from the delivery record: no header field is read, only the two
 * addresses are copied from where the record says they lie */
static void record_fill(const uint8_t *buf, const struct wc_rx_record *r, struct iov *i)
{
    memset(i, 0, sizeof *i);
    const unsigned alen = r->af == 4 ? 4 : 16;
    i->af = r->af;
    memcpy(i->addr, buf + r->src_off, alen);
    memcpy(i->local, buf + r->dst_off, alen);
    i->flags = r->tos;
    i->ttl = r->ttl;
    i->len = r->data_len;
    i->port = r->sport;
    i->lport = r->dport;
    i->base = buf;
    i->buf = buf + r->data_off;
}

#define FAIL(...) RING_FAIL("rx_deliver_loop", __VA_ARGS__)

int main(int argc, char **argv)
{
    const uint32_t nslots = argc > 1 ? (uint32_t)atoi(argv[1]) : 6000;
    const uint64_t mem_size = (uint64_t)nslots * BUF_SIZE;
    uint8_t *mem = aligned_alloc(4096, mem_size);
    struct nm_slot *slot = calloc(nslots, sizeof *slot);
    int *kind = malloc(nslots * sizeof *kind);
    uint64_t *off = malloc(nslots * sizeof *off);
    uint16_t *flen = malloc(nslots * sizeof *flen);
    uint8_t *verdict = malloc(nslots);
    struct wc_rx_record *rec = malloc(nslots * sizeof *rec);
    uint32_t *list = malloc(nslots * sizeof *list), *host_list = malloc(nslots * sizeof *list);
    if (!mem || !slot || !kind || !off || !flen || !verdict || !rec || !list || !host_list)
        FAIL("alloc");
    for (uint32_t i = 0; i < nslots; i++)
        slot[i].buf_idx = i;
    ring_shuffle(&slot[0].buf_idx, sizeof *slot, nslots);
    uint64_t delivered = 0, to_host = 0, dropped = 0;
    for (int pass = 0; pass < 2; pass++) {
        if (pass == 0 && wc_host_register(mem, mem_size) != WC_OK)
            FAIL("wc_host_register");
        if (pass == 1 && wc_host_unregister(mem) != WC_OK)
            FAIL("wc_host_unregister");
        for (uint32_t s = 0; s < nslots; s++) {
            kind[s] = (int)(rnd() % NCASES);
            slot[s].len = make_frame(mem + (uint64_t)slot[s].buf_idx * BUF_SIZE, kind[s]);
            off[s] = (uint64_t)slot[s].buf_idx * BUF_SIZE;
            flen[s] = slot[s].len;
        }
        memset(rec, 0xEE, nslots * sizeof *rec);
        uint64_t count = ~0ull, drops = ~0ull;
        const int rc = wc_rx_deliver_host(mem, mem_size, off, flen, nslots, verdict, rec, list,
                                          &count, &drops);
        if (rc != WC_OK)
            FAIL("wc_rx_deliver_host: %s (%d)", wc_strerror(rc), rc);
        /* the delivered frames: h_list only, the iov from the record */
        uint64_t k = 0;
        for (uint32_t s = 0; s < nslots; s++) {
            const uint8_t *buf = mem + off[s];
            if (verdict[s] != oracle_rx_verdict(buf, flen[s]))
                FAIL("slot %u: verdict %d, oracle %d", s, verdict[s],
                     oracle_rx_verdict(buf, flen[s]));
            if (!accepted(kind[s])) {
                static const struct wc_rx_record zero;
                if (memcmp(&rec[s], &zero, sizeof zero))
                    FAIL("slot %u (case %d): a record for a frame that is not delivered", s,
                         kind[s]);
                continue;
            }
            if (k >= count || list[k] != s)
                FAIL("slot %u (case %d) is accepted but is not entry %llu of the list", s,
                     kind[s], (unsigned long long)k);
            ++k;
        }
        if (k != count)
            FAIL("list of %llu entries for %llu accepted frames", (unsigned long long)count,
                 (unsigned long long)k);
        for (uint64_t q = 0; q < count; q++) {
            const uint32_t s = list[q];
            const uint8_t *buf = mem + off[s];
            struct iov a, b;
            record_fill(buf, &rec[s], &a);
            udp_rx_fill(buf, &b);
            if (memcmp(&a, &b, sizeof a))
                FAIL("slot %u (case %d): the iov from the record differs from udp_rx's "
                     "(len %u vs %u, af %u vs %u, flags %u vs %u, ttl %u vs %u, buf +%ld vs +%ld)",
                     s, kind[s], a.len, b.len, a.af, b.af, a.flags, b.flags, a.ttl, b.ttl,
                     (long)(a.buf - buf), (long)(b.buf - buf));
            ++delivered;
        }
        /* the host's frames: the WC_RX_MASK_HOST list over the verdict bytes */
        uint64_t nh = 0, nd = 0;
        for (uint32_t s = 0; s < nslots; s++) {
            if ((WC_RX_MASK_HOST >> verdict[s]) & 1u)
                host_list[nh++] = s;
            nd += WC_RX_IS_DROP(verdict[s]);
        }
        uint64_t h = 0;
        for (uint32_t s = 0; s < nslots; s++)
            if (hosts(kind[s]) && (h >= nh || host_list[h++] != s))
                FAIL("slot %u (case %d) is the host's but not in the host list", s, kind[s]);
        if (h != nh)
            FAIL("host list of %llu entries for %llu ARP / ICMP frames", (unsigned long long)nh,
                 (unsigned long long)h);
        if (nd != drops || nd + nh + count != nslots)
            FAIL("drops %llu vs %llu; %llu + %llu + %llu != %u", (unsigned long long)drops,
                 (unsigned long long)nd, (unsigned long long)nd, (unsigned long long)nh,
                 (unsigned long long)count, nslots);
        to_host += nh;
        dropped += nd;
    }
    wc_gpu_fini();
    printf("rx_deliver_loop: ok (%u slots, 2 passes: %llu delivered from records, %llu to the "
           "host stack, %llu dropped)\n",
           nslots, (unsigned long long)delivered, (unsigned long long)to_host,
           (unsigned long long)dropped);
    return 0;
}
