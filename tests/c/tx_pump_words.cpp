// tx_pump_words.cpp -- the TX pump's shared statement (warpcore_amd/csrc/
// wc_tx_pump.h: the per-frame gate, and the plan launch's destination steps over
// a set, a where array and a copy of the state bytes) compiled for the host
// alone and driven from a command file, so the lines the gfx950 kernels compile
// are held against tests/tx_pump_model.py without a GPU
// (tests/test_tx_pump_words.py).  The destinations of the plan launch are run
// one after the other, in an order the command file states for each of the two
// steps that a workgroup barrier separates.
//
// Commands (little-endian uint32 words unless stated):
//   1 INIT   cap                                        -> (nothing)
//   2 APPLY  m, m 24-byte records (applied in order)    -> dropped
//   3 GATE   k, k x (hold, sock_in, w0, dst_in, data_len, slot_bytes, zero_udp)
//            -> k x (the chain's status, its frame length, the gate's status,
//                    length, built, error)
//   4 PLAN   ndst, ndst 24-byte entries, ndst af bytes padded to a multiple of 4,
//            ndst indices (the find step's order), ndst indices (the mark step's)
//            -> the state bytes padded alike, the entries
#include <stdio.h>
#include <stdlib.h>
#include <vector>

#include "wc_tx_pump.h"

namespace tn = wc::tn;
namespace tp = wc::tp;
namespace txb = wc::txb;

static FILE *in, *out;

static void rd(void *p, size_t bytes)
{
    if (bytes && fread(p, 1, bytes, in) != bytes) {
        fprintf(stderr, "short command file\n");
        exit(2);
    }
}

static uint32_t rd32()
{
    uint32_t v;
    rd(&v, 4);
    return v;
}

static std::vector<uint32_t> rd_order(uint32_t n)
{
    std::vector<uint32_t> o(n);
    rd(o.data(), 4ull * n);
    std::vector<uint8_t> seen(n, 0);
    for (uint32_t x : o) {
        if (x >= n || seen[x]) {
            fprintf(stderr, "an order that is no permutation\n");
            exit(2);
        }
        seen[x] = 1;
    }
    return o;
}

static void wr(const void *p, size_t bytes)
{
    fwrite(p, 1, bytes, out);
}

int main(int argc, char **argv)
{
    if (argc != 3)
        return 2;
    in = fopen(argv[1], "rb"), out = fopen(argv[2], "wb");
    if (!in || !out)
        return 2;
    const tn::HostWords w{};
    std::vector<uint32_t> tab;
    uint32_t op;
    while (fread(&op, 4, 1, in) == 1) {
        if (op == 1) {
            const uint32_t cap = rd32();
            if (!tn::tab_bytes(cap))
                return 2;
            tab.assign(tn::tab_bytes(cap) / 4, 0u);
            tab[0] = tn::kTabMagic, tab[1] = cap;
        } else if (op == 2) {
            const uint32_t m = rd32();
            if (tab.empty() || m == 0)
                return 2;
            std::vector<uint32_t> upd(6ull * m), ent(m, 0xDEADBEEFu);
            rd(upd.data(), 24ull * m);
            const uint32_t cap = tn::tab_cap(w, tab.data());
            uint32_t dropped = 0;
            for (uint32_t j = 0; j < m; ++j) {
                bool drop;
                ent[j] = tn::apply_claim(w, tab.data(), cap, upd.data(), m, j, drop);
                dropped += drop;
            }
            for (uint32_t j = 0; j < m; ++j)
                tn::apply_commit(w, tab.data(), cap, upd.data(), j, ent[j]);
            wr(&dropped, 4);
        } else if (op == 3) {
            const uint32_t k = rd32();
            for (uint32_t q = 0; q < k; ++q) {
                uint32_t a[7];
                rd(a, sizeof a);
                const txb::Decide x = txb::decide(a[1] != 0, a[2], a[3] != 0, a[4], a[5], a[6] != 0);
                const tp::Gate g = tp::gate(a[0], x);
                const uint32_t res[6] = {x.status, x.flen, g.status, g.flen, g.built, g.error};
                wr(res, sizeof res);
            }
        } else if (op == 4) {
            const uint32_t ndst = rd32(), pad = (ndst + 3u) & ~3u;
            if (ndst == 0 || ndst > tp::kSmallDst || tab.empty())
                return 2;
            std::vector<uint32_t> dsts(6ull * ndst);
            std::vector<uint8_t> afs(pad), lstate(pad, 0xEEu);
            rd(dsts.data(), 24ull * ndst);
            rd(afs.data(), pad);
            const std::vector<uint32_t> o1 = rd_order(ndst), o2 = rd_order(ndst);
            const uint32_t cap = tn::tab_cap(w, tab.data());
            // exactly what the workgroup places: no word more
            std::vector<uint32_t> set(2ull * tn::set_slots(ndst), 0u), where(ndst, 0xDEADBEEFu);
            for (uint32_t k : o1) // ... barrier ...
                tp::dst_find(w, tab.data(), cap, dsts.data(), afs.data(), ndst, k, set.data(),
                             lstate.data(), where.data());
            for (uint32_t k : o2)
                tp::dst_mark(w, ndst, k, set.data(), lstate.data(), where.data());
            for (uint32_t k = ndst; k < pad; ++k)
                lstate[k] = 0;
            wr(lstate.data(), pad);
            wr(dsts.data(), 24ull * ndst);
        } else {
            return 2;
        }
    }
    fclose(out);
    return 0;
}
