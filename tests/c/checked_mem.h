// checked_mem.h -- the `Mem` the host "words" programs (tx_build_words.cpp,
// rx_reply_words.cpp, rx_neigh_words.cpp) hand to the shared frame statements
// of warpcore_amd/csrc: every access is checked before it is made, and a
// refused one ends the program with a message and exit status 3.  Loads must be
// aligned and overlap [flo, fhi) (the frame); stores must be naturally aligned
// and lie inside [lo, hi) (`what`, called `where` in offsets).
#pragma once

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

struct CheckedMem {
    uint64_t flo, fhi; // the frame: the only bytes a load may overlap
    uint64_t lo, hi;   // the only bytes a store may touch
    const char *where = "reply", *what = "the reply";
    void chk_ld(uint64_t a, unsigned w, const char *kind) const
    {
        if (a % w || a + w <= flo || a >= fhi) {
            fprintf(stderr, "%sload at frame%+lld: misaligned or outside the frame\n", kind,
                    (long long)(a - flo));
            exit(3);
        }
    }
    void chk(uint64_t a, unsigned w) const
    {
        if (a % w || a < lo || a + w > hi) {
            fprintf(stderr, "store of %u bytes at %s%+lld: misaligned or outside %s\n", w, where,
                    (long long)(a - lo), what);
            exit(3);
        }
    }
    uint32_t ld32(uint64_t a) const
    {
        chk_ld(a, 4, "");
        uint32_t v;
        memcpy(&v, (const void *)(uintptr_t)a, 4);
        return v;
    }
    void st32(uint64_t a, uint32_t v) const { chk(a, 4), memcpy((void *)(uintptr_t)a, &v, 4); }
    void st16(uint64_t a, uint32_t v) const
    {
        const uint16_t x = (uint16_t)v;
        chk(a, 2), memcpy((void *)(uintptr_t)a, &x, 2);
    }
    void st8(uint64_t a, uint32_t v) const { chk(a, 1), *(uint8_t *)(uintptr_t)a = (uint8_t)v; }
};

// The same with 16-byte chunks as a struct of four dwords (rr::Quad).
template <class Quad>
struct CheckedMem128 : CheckedMem {
    Quad ld128(uint64_t a) const
    {
        chk_ld(a, 16, "chunk ");
        Quad q;
        memcpy(&q, (const void *)(uintptr_t)a, 16);
        return q;
    }
    void st128(uint64_t a, const Quad &q) const
    {
        chk(a, 16), memcpy((void *)(uintptr_t)a, &q, 16);
    }
};

static inline uint32_t le32(const uint8_t *p)
{
    uint32_t v;
    memcpy(&v, p, 4);
    return v;
}
