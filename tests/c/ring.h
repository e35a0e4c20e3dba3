/*
 * ring.h -- what the ring loop programs (rx_ring_loop, rx_deliver_loop,
 * rx_demux_loop, tx_seal_loop, tx_queue_loop) share: the netmap-like slot,
 * the buffer size, the generator every ring is built from, and the failure
 * report.  Header-only; each program defines RING_SEED before including it,
 * so its rings are its own, and keeps its make_frame.
 */
#ifndef WC_TESTS_RING_H
#define WC_TESTS_RING_H

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#define BUF_SIZE 2048

/* netmap_slot, the fields w_nic_rx touches (netmap.h) */
struct nm_slot {
    uint32_t buf_idx;
    uint16_t len;
    uint16_t flags;
    uint64_t ptr;
};

static uint64_t rng = RING_SEED; /* xorshift64 */
static uint32_t rnd(void)
{
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return (uint32_t)(rng >> 11);
}

static void put16(uint8_t *p, uint16_t v) /* network order (bswap16 stores) */
{
    p[0] = (uint8_t)(v >> 8);
    p[1] = (uint8_t)v;
}

/* Fisher-Yates over the n uint32 values `stride` bytes apart from `first` on
 * (an index array, or the buf_idx of an array of slots): buffers handed out
 * in scrambled order (zero-copy swaps, w_alloc). */
static void ring_shuffle(void *first, size_t stride, uint32_t n)
{
    for (uint32_t i = n; i-- > 1;) {
        uint32_t *a = (uint32_t *)((char *)first + i * stride);
        uint32_t *b = (uint32_t *)((char *)first + (rnd() % (i + 1)) * stride);
        const uint32_t t = *a;
        *a = *b;
        *b = t;
    }
}

/* "<prog>: FAIL <message>" on stdout and `return 1` from the caller (main). */
#define RING_FAIL(prog, ...)                                                   \
    do {                                                                       \
        printf(prog ": FAIL ");                                                \
        printf(__VA_ARGS__);                                                   \
        printf("\n");                                                          \
        return 1;                                                              \
    } while (0)

#endif
