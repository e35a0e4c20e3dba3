// rx_answer_words.cpp -- the RX answer's shared statements compiled for the host
// alone (tests/test_rx_answer_words.py): the grid split of its frames launch
// (warpcore_amd/csrc/wc_rx_answer.h) over a whole cube of list sizes, and the
// claim and commit steps of its apply launch run through wc_tx_neigh.h with the
// host Words, the lanes of the one workgroup visited in an order the command
// file states and the entry index kept in a local array, next to the two-launch
// form of tx_neigh_words.cpp with its scratch array.
//
// Commands (little-endian uint32 words unless stated):
//   1 INIT    cap                                        -> (nothing)
//   2 APPLY   m, lim, m 24-byte records, lim record indices (the claim launch's
//             order), lim indices (the commit launch's)  -> dropped
//   3 LOOKUP  nq, nq x (af, 16 address bytes)            -> nq x (hit, 8 bytes: the MAC, 0 0)
//   4 STATS                                              -> cap, used, entries whose last is not 0,
//                                                           entries neither empty nor full
//   5 DUMP                                               -> the table's words
//   6 SPLIT   (the cube is the program's own)            -> cases checked, the largest grid
//   7 ANSWER  u_m, count, u_m 24-byte records, 4096 visit numbers (step B's
//             order), 4096 visit numbers (step C's)      -> dropped
//             visit v = (step, wave, lane) in the order the hardware would run
//             them with all waves in lock step: v = (step * 16 + wave) * 64 + lane
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "wc_rx_answer.h"
#include "wc_tx_neigh.h"

namespace tn = wc::tn;
namespace ra = wc::ra;

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

static void fail(const char *what, uint32_t r, uint32_t n, uint32_t u, uint32_t cap)
{
    fprintf(stderr, "split(%u, %u, %u, cap %u): %s\n", r, n, u, cap, what);
    exit(3);
}

// Every entry j < m of a role visited exactly once by its workgroups' strides.
template <class First, class Step>
static void visit(std::vector<uint8_t> &seen, uint32_t m, uint32_t count, uint32_t per, First first,
                  Step step, const char *what, uint32_t r, uint32_t n, uint32_t u, uint32_t cap)
{
    seen.assign(m, 0);
    for (uint32_t rank = 0; rank < count; ++rank)
        for (uint32_t t = 0; t < per; ++t)
            for (uint64_t j = first(rank, t); j < m; j += step(count))
                if (seen[j]++)
                    fail(what, r, n, u, cap);
    for (uint32_t j = 0; j < m; ++j)
        if (seen[j] != 1)
            fail(what, r, n, u, cap);
}

static void split_cube(uint32_t res[2])
{
    static const uint32_t ms[] = {0, 1, 63, 64, 65, 255, 256, 257, 4095, 4096};
    static const uint32_t cus[] = {1, 8, 256};
    static const uint32_t per_cu[] = {1, 2, 8};
    std::vector<uint8_t> seen;
    res[0] = res[1] = 0;
    for (uint32_t c : cus)
        for (uint32_t p : per_cu)
            for (uint32_t r : ms)
                for (uint32_t n : ms)
                    for (uint32_t u : ms) {
                        const uint32_t cap = ra::grid_cap(c, p);
                        const ra::Split s = ra::split(r, n, u, cap);
                        const uint32_t grid = ra::grid_of(s);
                        if ((grid == 0) != (r == 0 && n == 0 && u == 0))
                            fail("an empty grid, or one for nothing", r, n, u, cap);
                        if (grid > cap || cap < 3 || (uint64_t)cap < (uint64_t)c * p)
                            fail("the grid exceeds the cap", r, n, u, cap);
                        if ((s.gr == 0) != (r == 0) || (s.gn == 0) != (n == 0) || (s.gu == 0) != (u == 0))
                            fail("a role without a workgroup, or one without work", r, n, u, cap);
                        // every workgroup has exactly one role, and the roles tile the grid
                        uint32_t count[3] = {0, 0, 0};
                        for (uint32_t b = 0; b < grid; ++b) {
                            const ra::Role ro = ra::role_of(s, b);
                            if (ro.kind > 2 || b < ro.first || b - ro.first >= ro.count)
                                fail("a workgroup outside its role", r, n, u, cap);
                            const uint32_t want = ro.kind == ra::kRoleReply   ? s.gr
                                                  : ro.kind == ra::kRoleNeigh ? s.gn
                                                                              : s.gu;
                            if (ro.count != want)
                                fail("a role's count", r, n, u, cap);
                            ++count[ro.kind];
                        }
                        if (count[0] != s.gr || count[1] != s.gn || count[2] != s.gu)
                            fail("the roles do not tile the grid", r, n, u, cap);
                        visit(seen, r, s.gr, ra::kWaves, ra::first_reply, ra::reply_step, "replies", r,
                              n, u, cap);
                        visit(seen, n, s.gn, ra::kThreads, ra::first_entry, ra::entry_step,
                              "neighbour replies", r, n, u, cap);
                        visit(seen, u, s.gu, ra::kThreads, ra::first_entry, ra::entry_step, "records",
                              r, n, u, cap);
                        ++res[0];
                        res[1] = grid > res[1] ? grid : res[1];
                    }
}

// Visit v of the apply workgroup -> the entry its lane takes in that step.
static uint32_t entry_of_visit(uint32_t v)
{
    const uint32_t lane = v & 63u, wave = (v >> 6) % ra::kApplyWaves;
    const uint32_t step = (v >> 6) / ra::kApplyWaves;
    return ra::apply_index(wave, step, lane);
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
            wr(tab.data(), 4 * tab.size());
        } else if (op == 6) {
            uint32_t res[2];
            split_cube(res);
            wr(res, 8);
        } else if (op == 7) {
            const uint32_t u_m = rd32(), count = rd32();
            if (u_m == 0 || u_m > ra::kSmall || tab.empty())
                return 2;
            std::vector<uint32_t> upd(6ull * u_m);
            rd(upd.data(), 24ull * u_m);
            const std::vector<uint32_t> o1 = rd_order(ra::kSmall, ra::kSmall),
                                        o2 = rd_order(ra::kSmall, ra::kSmall);
            // k_rx_answer_apply's steps B and C: the index in a local array
            uint32_t ent[ra::kSmall];
            for (uint32_t &e : ent)
                e = 0xDEADBEEFu;
            const uint32_t lim = count < u_m ? count : u_m;
            const uint32_t cap = tn::tab_cap(w, tab.data());
            uint32_t dropped = 0;
            for (uint32_t v : o1) {
                const uint32_t k = entry_of_visit(v);
                bool drop = false;
                if (k < lim)
                    ent[k] = tn::apply_claim(w, tab.data(), cap, upd.data(), lim, k, drop);
                dropped += drop;
            }
            for (uint32_t v : o2) {
                const uint32_t k = entry_of_visit(v);
                if (k < lim)
                    tn::apply_commit(w, tab.data(), cap, upd.data(), k, ent[k]);
            }
            wr(&dropped, 4);
        } else {
            return 2;
        }
    }
    fclose(out);
    return 0;
}
