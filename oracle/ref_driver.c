/*
 * ref_driver.c -- TEST INFRASTRUCTURE ONLY.
 *
 * Batch driver linked into oracle/_ref/libwc_ref.so beside the reference's
 * own in_cksum.c (oracle/Makefile, target `ref`): it loops a ragged batch
 * over the reference's two functions, which that build renames to
 * wcref_ip_cksum / wcref_payload_cksum.  This file holds no checksum
 * arithmetic of its own -- every value comes out of the reference's object.
 *
 * payload_cksum(buf, len) with len below the IP header length is not defined
 * in the reference (len - hl becomes a uint32 near 2^32: a ~4 GiB read), so
 * such a call is refused here, never made.
 */
#include <stdint.h>

uint16_t wcref_ip_cksum(const void *buf, uint16_t len);
uint16_t wcref_payload_cksum(const void *buf, uint16_t len);

enum { WCREF_KIND_IP = 0, WCREF_KIND_PAYLOAD = 1 };

/* The header length payload_cksum takes from the first byte: 4 * IHL where
 * the version nibble is 4, the 40-byte IPv6 header for every other nibble. */
static uint32_t hdr_len(const uint8_t *p)
{
    return (p[0] >> 4) == 4 ? (uint32_t)(p[0] & 0x0Fu) * 4u : 40u;
}

/* 0 and *out on success; -1 (and no call into the reference) for len < hl. */
int wcref_payload_cksum_checked(const uint8_t *buf, uint16_t len, uint16_t *out)
{
    if (len < hdr_len(buf))
        return -1;
    *out = wcref_payload_cksum(buf, len);
    return 0;
}

/* out[i] = cksum(base + off[i], len[i]).  Returns -1 on success.  A payload
 * batch is scanned first: if packet i has len < hl, i is returned and nothing
 * is computed. */
int64_t wcref_cksum_ragged(const uint8_t *base, const uint64_t *off, const uint16_t *len,
                           uint64_t n, uint16_t *out, int kind)
{
    if (kind == WCREF_KIND_PAYLOAD)
        for (uint64_t i = 0; i < n; i++)
            if (len[i] < hdr_len(base + off[i]))
                return (int64_t)i;
    for (uint64_t i = 0; i < n; i++)
        out[i] = kind == WCREF_KIND_PAYLOAD ? wcref_payload_cksum(base + off[i], len[i])
                                            : wcref_ip_cksum(base + off[i], len[i]);
    return -1;
}
