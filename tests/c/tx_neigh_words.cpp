// tx_neigh_words.cpp -- the TX neighbours' shared statement (warpcore_amd/csrc/
// wc_tx_neigh.h: table layout, hash, probe / claim / commit, lookup, resolve and
// its de-duplication, both solicitation frames and their stores at any phase)
// compiled for the host alone and driven from a command file, so the lines the
// gfx950 kernels compile are held against tests/tx_neigh_model.py without a GPU
// (tests/test_tx_neigh_words.py).  The lanes of a launch are run one after the
// other in an order the command file states, launch by launch.
//
// Commands (little-endian uint32 words unless stated):
//   1 INIT    cap                         -> (nothing)
//   2 APPLY   m, lim, m 24-byte records, lim indices (the claim launch's order),
//             lim indices (the commit launch's order)   -> dropped
//   3 LOOKUP  nq, nq x (af, 16 address bytes)           -> nq x (hit, 8 bytes: the MAC, 0 0)
//   4 STATS                                             -> cap, used, entries whose last is not 0,
//                                                          entries neither empty nor full
//   5 RESOLVE ndst, ndst 24-byte entries, ndst af bytes padded to a multiple of
//             4, ndst indices (the find launch's order), ndst indices (the mark
//             launch's)                   -> the state bytes padded alike, the entries
//   6 SOLICIT the 844 table bytes, af, 16 address bytes, slot_bytes, phase
//                                         -> length, a 256-byte region pre-filled
//                                            with 0xA5, the frame at byte 16 + phase
// Every frame store is checked (checked_mem.h): naturally aligned and inside the
// frame.
#include <vector>

#include "checked_mem.h"
#include "wc_tx_neigh.h"

namespace tn = wc::tn;
namespace rr = wc::rr;

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

static std::vector<uint32_t> rd_order(uint32_t n, uint32_t below)
{
    std::vector<uint32_t> o(n);
    rd(o.data(), 4ull * n);
    for (uint32_t x : o)
        if (x >= below) {
            fprintf(stderr, "an order entry past the launch\n");
            exit(2);
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
            const uint32_t m = rd32(), lim = rd32();
            if (lim > m || tab.empty())
                return 2;
            std::vector<uint32_t> upd(6ull * m), ent(m, 0xDEADBEEFu);
            rd(upd.data(), 24ull * m);
            const std::vector<uint32_t> o1 = rd_order(lim, lim), o2 = rd_order(lim, lim);
            const uint32_t cap = tn::tab_cap(w, tab.data());
            uint32_t dropped = 0;
            for (uint32_t j : o1) {
                bool drop;
                ent[j] = tn::apply_claim(w, tab.data(), cap, upd.data(), lim, j, drop);
                dropped += drop;
            }
            for (uint32_t j : o2)
                tn::apply_commit(w, tab.data(), cap, upd.data(), j, ent[j]);
            wr(&dropped, 4);
        } else if (op == 3) {
            const uint32_t nq = rd32(), cap = tn::tab_cap(w, tab.data());
            for (uint32_t q = 0; q < nq; ++q) {
                uint32_t a[5];
                rd(a, 20);
                uint32_t m0 = 0, m1 = 0;
                const uint32_t res[3] = {
                    tn::lookup(w, tab.data(), cap, tn::key_of(a[0], a[1], a[2], a[3], a[4]), m0, m1),
                    m0, m1};
                wr(res, 12);
            }
        } else if (op == 4) {
            const uint32_t cap = tn::tab_cap(w, tab.data());
            uint32_t res[4] = {cap, 0u, 0u, 0u};
            for (uint32_t s = 0; s < cap; ++s) {
                const uint32_t *e = tn::tab_entry(tab.data(), s);
                res[1] += e[0] == tn::kFull;
                res[2] += e[1] != 0u;
                res[3] += e[0] != tn::kFull && e[0] != tn::kEmpty;
            }
            wr(res, 16);
        } else if (op == 5) {
            const uint32_t ndst = rd32(), pad = (ndst + 3u) & ~3u;
            if (ndst == 0 || ndst > tn::kResolveMax)
                return 2;
            std::vector<uint32_t> dsts(6ull * ndst);
            std::vector<uint8_t> afs(pad), state(pad, 0xEEu);
            rd(dsts.data(), 24ull * ndst);
            rd(afs.data(), pad);
            const std::vector<uint32_t> o1 = rd_order(ndst, ndst), o2 = rd_order(ndst, ndst);
            const uint32_t slots = tn::set_slots(ndst), cap = tn::tab_cap(w, tab.data());
            std::vector<uint32_t> set(2ull * slots, 0u), where(ndst, 0xDEADBEEFu);
            for (uint32_t k : o1)
                tn::resolve_find(w, tab.data(), cap, dsts.data(), afs.data(), ndst, k, set.data(), slots,
                                 state.data(), where.data());
            for (uint32_t k : o2)
                tn::resolve_mark(w, k, set.data(), slots, state.data(), where.data());
            for (uint32_t k = ndst; k < pad; ++k)
                state[k] = 0;
            wr(state.data(), pad);
            wr(dsts.data(), 24ull * ndst);
        } else if (op == 6) {
            alignas(16) static uint8_t region[256];
            uint32_t e[rr::kEngineWords], arg[7];
            rd(e, 4 * rr::kEngineWords);
            rd(arg, 28);
            const uint32_t af = arg[0], slot = arg[5], dp = arg[6];
            if (dp > 15)
                return 2;
            const uint32_t t[4] = {arg[1], arg[2], arg[3], arg[4]};
            memset(region, 0xA5, sizeof region);
            const uint64_t da = (uint64_t)(uintptr_t)region + 16u + dp;
            // the bounds on their own: the stores may touch this much and no more
            const uint32_t most = af == 4 ? (slot >= 42 ? 42u : 0u) : af == 6 ? (slot >= 86 ? 86u : 0u) : 0u;
            CheckedMem mem{0, 0, da, da + most};
            mem.where = "frame", mem.what = "the frame";
            const uint32_t len = tn::solicit(mem, t, af, e, da, slot);
            if (len != 0 && len != most) {
                fprintf(stderr, "length %u where %u or 0 is due\n", len, most);
                exit(3);
            }
            wr(&len, 4);
            wr(region, sizeof region);
        } else {
            return 2;
        }
    }
    fclose(out);
    return 0;
}
