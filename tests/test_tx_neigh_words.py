"""CPU test of the lines the TX neighbour kernels compile
(warpcore_amd/csrc/wc_tx_neigh.h), compiled for the host alone
(tests/c/tx_neigh_words.cpp, with -fsanitize=address,undefined, run directly):
the table's apply with the records visited in shuffled and reversed orders, a
small table whose probes wrap, the full-table rule, a second apply on the same
table, resolve's de-duplication under shuffled orders, and both solicitation
frames at all 16 destination phases -- all against tests/tx_neigh_model.py.  The
program itself refuses a frame store that is misaligned or leaves the frame."""
import struct
import subprocess

import numpy as np
import pytest

import cprog
import rx_reply_cases as rc
import tx_neigh_cases as cases
import tx_neigh_model as model

REGION = 256


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return cprog.build_words("tx_neigh_words", tmp_path_factory.mktemp("txn"))


class Script:
    """A command file and the parser of the program's answers, in order."""

    def __init__(self):
        self.blob, self.readers = bytearray(), []

    def init(self, cap):
        self.blob += struct.pack("<2I", 1, cap)

    def apply(self, upd: np.ndarray, lim: int, o1, o2):
        m = upd.size
        self.blob += struct.pack("<3I", 2, m, lim) + upd.tobytes()
        self.blob += np.asarray(o1, np.uint32).tobytes() + np.asarray(o2, np.uint32).tobytes()
        self.readers.append((4, lambda b: struct.unpack("<I", b)[0]))

    def lookup(self, ks):
        self.blob += struct.pack("<2I", 3, len(ks))
        for af, a in ks:
            a = bytes(a[:4]) + bytes(12) if af == 4 else bytes(a)
            self.blob += struct.pack("<I", af) + a
        def parse(b):
            out = []
            for q in range(len(ks)):
                hit, = struct.unpack("<I", b[12 * q:12 * q + 4])
                out.append(b[12 * q + 4:12 * q + 10] if hit else None)
            return out
        self.readers.append((12 * len(ks), parse))

    def stats(self):
        self.blob += struct.pack("<I", 4)
        self.readers.append((16, lambda b: struct.unpack("<4I", b)))

    def resolve(self, dsts: np.ndarray, afs: np.ndarray, o1, o2):
        n, pad = dsts.size, (dsts.size + 3) & ~3
        self.blob += struct.pack("<2I", 5, n) + dsts.tobytes() + afs.tobytes() + bytes(pad - n)
        self.blob += np.asarray(o1, np.uint32).tobytes() + np.asarray(o2, np.uint32).tobytes()
        self.readers.append((pad + 24 * n, lambda b: (np.frombuffer(b[:n], np.uint8),
                                                      np.frombuffer(b[pad:], model.DST))))

    def solicit(self, eng, af, addr, slot, dp):
        a = (bytes(addr) + bytes(16))[:16]
        self.blob += struct.pack("<I", 6) + eng.tobytes() + struct.pack("<I", af) + a + \
            struct.pack("<2I", slot, dp)
        self.readers.append((4 + REGION, lambda b: (struct.unpack("<I", b[:4])[0], b[4:])))

    def run(self, exe, tmp_path):
        src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
        src.write_bytes(bytes(self.blob))
        r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
        raw, at, out = dst.read_bytes(), 0, []
        for size, parse in self.readers:
            out.append(parse(raw[at:at + size]))
            at += size
        assert at == len(raw)
        return out


def orders(n, k=4, seed=1):
    """In order, reversed, and k shuffles -- as (claim order, commit order)."""
    rng = np.random.default_rng(seed)
    ident = np.arange(n, dtype=np.uint32)
    out = [(ident, ident), (ident[::-1], ident[::-1]), (ident, ident[::-1])]
    out += [(rng.permutation(n), rng.permutation(n)) for _ in range(k)]
    return out


def want_lookups(cache, ks):
    return [cache.get(model.key(af, a)) for af, a in ks]


@pytest.mark.parametrize("name", list(cases.WORLDS))
def test_apply_in_any_order_is_the_in_order_result(exe, tmp_path, name):
    seed, n, nkeys = cases.WORLDS[name]
    recs, ks = cases.record_world(seed, n, nkeys)
    upd = model.records(recs)
    probe = ks + [(4, cases.addr4(9999)), (6, cases.addr6(9999))]
    for lim in (n, n - 37):
        cache = {}
        dropped = model.apply(cache, upd, lim, n)
        assert dropped > 5 and len(cache) == len(ks)
        s = Script()
        for o1, o2 in orders(lim, seed=seed):
            s.init(256)
            s.apply(upd, lim, o1, o2)
            s.lookup(probe)
            s.stats()
        got = s.run(exe, tmp_path)
        for i in range(0, len(got), 3):
            assert got[i] == dropped
            assert got[i + 1] == want_lookups(cache, probe)
            assert got[i + 2] == (256, len(cache), 0, 0)  # no stale last word, no claim left


def test_forty_keys_whose_probes_wrap_a_table_of_64(exe, tmp_path):
    ks = cases.wrap_keys(64, 40)  # all at home in the last 8 entries
    rng = np.random.default_rng(8)
    recs = [(af, cases.mac_of(rng), a) for af, a in ks] * 2
    recs += [(af, cases.mac_of(rng), a) for af, a in ks[:10]]
    upd = model.records(recs)
    cache = {}
    assert model.apply(cache, upd, len(recs), len(recs)) == 0
    s = Script()
    for o1, o2 in orders(len(recs), seed=2):
        s.init(64)
        s.apply(upd, len(recs), o1, o2)
        s.lookup(ks + cases.lookalikes())
        s.stats()
    got = s.run(exe, tmp_path)
    for i in range(0, len(got), 3):
        assert got[i] == 0
        assert got[i + 1] == want_lookups(cache, ks) + [None, None]
        assert got[i + 2] == (64, 40, 0, 0)


def test_probes_wrap_the_tables_end(exe, tmp_path):
    """Fill a 64-entry table to 63 keys one apply at a time: whatever the hash,
    the runs of full entries then cross the table's end, and every key is still
    found, as is the one free entry by a last key."""
    ks = cases.keys(64)
    rng = np.random.default_rng(4)
    recs = [(af, cases.mac_of(rng), a) for af, a in ks]
    s = Script()
    s.init(64)
    cache, want = {}, []
    for lo, hi in ((0, 30), (30, 63), (63, 64)):
        upd = model.records(recs[lo:hi])
        model.apply(cache, upd, hi - lo, hi - lo)
        o = np.random.default_rng(lo).permutation(hi - lo)
        s.apply(upd, hi - lo, o, o[::-1])
        s.lookup(ks)
        s.stats()
        want += [0, want_lookups(cache, ks), (64, hi, 0, 0)]
    assert s.run(exe, tmp_path) == want


def test_full_table_rule(exe, tmp_path):
    """80 distinct keys into 64 entries, each three times: 64 keys present,
    every present key with its last MAC, dropped = the records of absent keys;
    then a second apply that overwrites present keys and still cannot insert."""
    ks = cases.keys(80)
    rng = np.random.default_rng(6)
    recs = [(af, cases.mac_of(rng), a) for _ in range(3) for af, a in ks]
    rng.shuffle(recs)
    recs = [tuple(r) for r in recs]
    upd = model.records(recs)
    last = {}
    model.apply(last, upd, len(recs), len(recs))
    again = model.records([(af, cases.mac_of(rng), a) for af, a in ks])
    last2 = dict(last)
    model.apply(last2, again, 80, 80)
    s = Script()
    for o1, o2 in orders(len(recs), seed=9):
        s.init(64)
        s.apply(upd, len(recs), o1, o2)
        s.lookup(ks)
        s.stats()
        s.apply(again, 80, np.arange(80)[::-1], np.arange(80))
        s.lookup(ks)
        s.stats()
    got = s.run(exe, tmp_path)
    for i in range(0, len(got), 6):
        dropped, look, stats, dropped2, look2, stats2 = got[i:i + 6]
        present = [k for k, mac in zip(ks, look) if mac is not None]
        assert len(present) == 64 and stats == (64, 64, 0, 0) == stats2
        assert dropped == 3 * (80 - 64) and dropped2 == 80 - 64
        for (af, a), mac, mac2 in zip(ks, look, look2):
            assert (mac is None) == (mac2 is None)
            if mac is not None:
                assert mac == last[model.key(af, a)] and mac2 == last2[model.key(af, a)]


def test_second_and_third_apply_on_one_table(exe, tmp_path):
    """A stale last word or a leftover claim would show in the later applies."""
    seed, n, nkeys = cases.WORLDS["small"]
    recs, ks = cases.record_world(seed, n, nkeys)
    cache, s = {}, Script()
    s.init(128)
    want = []
    for r in range(3):
        part = model.records(recs[r * 100:(r + 1) * 100])
        want.append(model.apply(cache, part, 100, 100))
        o = np.random.default_rng(r).permutation(100)
        s.apply(part, 100, o, o[::-1])
        s.lookup(ks)
        want.append(want_lookups(cache, ks))
        s.stats()
        want.append((128, len(cache), 0, 0))
    assert s.run(exe, tmp_path) == want


@pytest.mark.parametrize("ndst", [1, 63, 64, 65, 257])
def test_resolve_and_its_deduplication_in_any_order(exe, tmp_path, ndst):
    recs, ks = cases.record_world(21, 200, 30)
    bc = (4, cases.addr4(77) + bytes(12))  # a cached broadcast MAC is unresolved
    recs.append((4, model.BCAST, bc[1]))
    upd = model.records(recs)
    cache = {}
    model.apply(cache, upd, len(recs), len(recs))
    dsts, afs = cases.dst_world(ndst, ndst, ks + [bc])
    state, after, lst = model.resolve(cache, dsts, afs)
    s = Script()
    s.init(256)
    s.apply(upd, len(recs), np.arange(len(recs)), np.arange(len(recs)))
    for o1, o2 in orders(ndst, seed=ndst):
        s.resolve(dsts, afs, o1, o2)
    got = s.run(exe, tmp_path)
    for g_state, g_dsts in got[1:]:
        assert (g_state == state).all()
        assert g_dsts.tobytes() == after.tobytes()
    if ndst >= 63:
        assert {int(x) for x in state} == {model.READY, model.BAD_AF, model.MISS, model.MISS_DUP}
        assert (after["port"] == dsts["port"]).all() and (after["addr"] == dsts["addr"]).all()


def test_both_frames_at_every_phase_and_slot_size(exe, tmp_path):
    eng = rc.engine_table()
    items = [(eng, af, a, slot, dp) for dp in range(16)
             for af, a in ((4, cases.PEER4), (6, cases.PEER6), (7, cases.PEER6), (0, cases.PEER4))
             for slot in (0, 41, 42, 43, 85, 86, 87)]
    items += [(e, af, a, 2048, 5) for e in (rc.engine_table(v4=0), rc.engine_table(v6=0),
                                            rc.engine_table(v4=0, v6=0))
              for af, a in ((4, cases.PEER4), (6, cases.PEER6))]
    rng = np.random.default_rng(3)
    items += [(rc.engine_table(rng=rng), af, rng.integers(0, 256, 16, dtype=np.uint8).tobytes(),
               int(rng.integers(80, 100)), int(rng.integers(0, 16)))
              for af in (4, 6) for _ in range(40)]
    s = Script()
    for it in items:
        s.solicit(*it)
    got = s.run(exe, tmp_path)
    lens = set()
    for (ln, region), (e, af, a, slot, dp) in zip(got, items):
        fr = model.solicit(af, a, e)
        if fr is not None and len(fr) > slot:
            fr = None
        want = bytearray(b"\xa5" * REGION)
        if fr is not None:
            want[16 + dp:16 + dp + len(fr)] = fr
        assert ln == (len(fr) if fr else 0) and region == bytes(want), (af, slot, dp)
        lens.add((af, ln))
    assert lens >= {(4, 0), (4, 42), (6, 0), (6, 86), (7, 0), (0, 0)}
    by = {(it[1], it[3], it[4]): g for g, it in zip(got, items[:16 * 28])}
    for dp in range(16):
        assert by[(4, 42, dp)][1][16 + dp:16 + dp + 42].hex() == cases.ARP_WHO_HAS_HEX
        assert by[(6, 86, dp)][1][16 + dp:16 + dp + 86].hex() == cases.NSOL_HEX
