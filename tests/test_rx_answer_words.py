"""CPU test of the lines the RX answer's two launches compile for host and
device alike (warpcore_amd/csrc/wc_rx_answer.h, and wc_tx_neigh.h's claim and
commit steps), compiled for the host alone (tests/c/rx_answer_words.cpp, with
-fsanitize=address,undefined, run directly).

The grid split: for every (r_m, n_m, u_m) in {0, 1, 63, 64, 65, 255, 256, 257,
4095, 4096}^3 and 1, 8 and 256 compute units, every workgroup has exactly one
role, every entry of each list is visited exactly once by its role's stride, the
grid is 0 only where every m is, and it never exceeds the cap (the program's own
checks; it exits non-zero at the first miss).

The apply launch's steps B and C: the lanes of the one workgroup in wave-step
order, reversed and shuffled, the entry index in a local array -- the table
must be byte for byte that of the two-launch form run in the same record order
with its scratch array, and the lookups those of tests/tx_neigh_model.py's
in-order apply."""
import struct
import subprocess

import numpy as np
import pytest

import cprog
import tx_neigh_cases as cases
import tx_neigh_model as model

SMALL, WAVES, STEPS = 4096, 16, 4


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return cprog.build_words("rx_answer_words", tmp_path_factory.mktemp("rxa"))


class Script:
    """A command file and the parser of the program's answers, in order."""

    def __init__(self):
        self.blob, self.readers = bytearray(), []

    def init(self, cap):
        self.blob += struct.pack("<2I", 1, cap)
        self.cap = cap

    def apply(self, upd: np.ndarray, lim: int, o1, o2):
        self.blob += struct.pack("<3I", 2, upd.size, lim) + upd.tobytes()
        self.blob += np.asarray(o1, np.uint32).tobytes() + np.asarray(o2, np.uint32).tobytes()
        self.readers.append((4, lambda b: struct.unpack("<I", b)[0]))

    def lookup(self, ks):
        self.blob += struct.pack("<2I", 3, len(ks))
        for af, a in ks:
            a = bytes(a[:4]) + bytes(12) if af == 4 else bytes(a)
            self.blob += struct.pack("<I", af) + a

        def parse(b):
            return [b[12 * q + 4:12 * q + 10] if struct.unpack("<I", b[12 * q:12 * q + 4])[0]
                    else None for q in range(len(ks))]
        self.readers.append((12 * len(ks), parse))

    def stats(self):
        self.blob += struct.pack("<I", 4)
        self.readers.append((16, lambda b: struct.unpack("<4I", b)))

    def dump(self):
        self.blob += struct.pack("<I", 5)
        self.readers.append((64 + 32 * self.cap, bytes))

    def split(self):
        self.blob += struct.pack("<I", 6)
        self.readers.append((8, lambda b: struct.unpack("<2I", b)))

    def answer(self, upd: np.ndarray, count: int, v1, v2):
        self.blob += struct.pack("<3I", 7, upd.size, count) + upd.tobytes()
        self.blob += np.asarray(v1, np.uint32).tobytes() + np.asarray(v2, np.uint32).tobytes()
        self.readers.append((4, lambda b: struct.unpack("<I", b)[0]))

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


def test_grid_split_over_the_cube(exe, tmp_path):
    s = Script()
    s.split()
    (ncases, largest), = s.run(exe, tmp_path)
    assert ncases == 3 * 3 * 10 ** 3  # CU counts x workgroups per CU x the cube
    assert largest == 1024 + 16 + 16   # 4096 replies at four per workgroup, uncapped at 256 x 8


def entry_of_visit(v):
    """The program's (and the kernel's) map: visit (step, wave, lane) -> entry."""
    v = np.asarray(v, np.int64)
    lane, wave, step = v & 63, (v >> 6) % WAVES, (v >> 6) // WAVES
    return wave * (64 * STEPS) + 64 * step + lane


def visit_orders(seed):
    """Wave-step order, reversed, and shuffles -- as (step B's, step C's)."""
    rng = np.random.default_rng(seed)
    ident = np.arange(SMALL, dtype=np.uint32)
    out = [(ident, ident), (ident[::-1], ident[::-1]), (ident, ident[::-1])]
    out += [(rng.permutation(SMALL), rng.permutation(SMALL)) for _ in range(3)]
    return out


def record_order(visits, lim):
    k = entry_of_visit(visits)
    return k[k < lim].astype(np.uint32)


def test_visits_reach_every_entry_once():
    k = entry_of_visit(np.arange(SMALL))
    assert sorted(k.tolist()) == list(range(SMALL))
    assert k[:64].tolist() == list(range(64)) and k[64] == 256 and k[64 * WAVES] == 64


def both_forms(s, cap, applies, v1, v2, probe):
    """The same applies on a fresh table in the answer's form, then in the
    two-launch form in the same record order; each followed by lookups, stats
    and the table's bytes."""
    for form in ("answer", "chain"):
        s.init(cap)
        for upd, count in applies:
            lim = min(count, upd.size)
            if form == "answer":
                s.answer(upd, count, v1, v2)
            else:
                s.apply(upd, lim, record_order(v1, lim), record_order(v2, lim))
        s.lookup(probe)
        s.stats()
        s.dump()


def check_forms(got, napplies, want_dropped, want_look, want_stats):
    per = napplies + 3
    for i in range(0, len(got), 2 * per):
        a, c = got[i:i + per], got[i + per:i + 2 * per]
        assert a[:napplies] == c[:napplies] == want_dropped
        assert a[napplies] == c[napplies] == want_look
        assert a[napplies + 1] == c[napplies + 1] == want_stats
        assert a[napplies + 2] == c[napplies + 2], "the table differs from the two-launch form's"


def test_wrapping_keys_in_a_table_of_64(exe, tmp_path):
    ks = cases.wrap_keys(64, 40)  # all at home in the last 8 entries
    rng = np.random.default_rng(8)
    recs = [(af, cases.mac_of(rng), a) for af, a in ks] * 2
    recs += [(af, cases.mac_of(rng), a) for af, a in ks[:10]]
    upd = model.records(recs)
    cache = {}
    assert model.apply(cache, upd, len(recs), len(recs)) == 0
    probe = ks + cases.lookalikes()
    s = Script()
    for v1, v2 in visit_orders(2):
        both_forms(s, 64, [(upd, len(recs) + 9)], v1, v2, probe)  # (a count past u_m)
    check_forms(s.run(exe, tmp_path), 1, [0],
                [cache.get(model.key(af, a)) for af, a in ks] + [None, None], (64, 40, 0, 0))


def test_eighty_keys_into_64_entries(exe, tmp_path):
    """The full-table rule: 64 keys present, each with its last MAC, dropped =
    the records of absent keys -- whichever keys the order lets in; the table is
    still that of the two-launch form in the same order."""
    ks = cases.keys(80)
    rng = np.random.default_rng(6)
    recs = [(af, cases.mac_of(rng), a) for _ in range(3) for af, a in ks]
    rng.shuffle(recs)
    upd = model.records([tuple(r) for r in recs])
    last = {}
    model.apply(last, upd, len(recs), len(recs))
    s = Script()
    for v1, v2 in visit_orders(9):
        both_forms(s, 64, [(upd, len(recs))], v1, v2, ks)
    got = s.run(exe, tmp_path)
    for i in range(0, len(got), 8):
        (dropped, look, stats, table), chain = got[i:i + 4], got[i + 4:i + 8]
        assert [dropped, look, stats, table] == chain
        assert stats == (64, 64, 0, 0) and dropped == 3 * (80 - 64)
        assert sum(mac is not None for mac in look) == 64
        for (af, a), mac in zip(ks, look):
            assert mac is None or mac == last[model.key(af, a)]


def test_second_apply_on_the_same_table(exe, tmp_path):
    """A stale last word or a leftover claim would show in the second apply."""
    seed, n, nkeys = cases.WORLDS["small"]
    recs, ks = cases.record_world(seed, n, nkeys)
    parts = [model.records(recs[:150]), model.records(recs[150:300])]
    cache = {}
    dropped = [model.apply(cache, p, 150, 150) for p in parts]
    s = Script()
    for v1, v2 in visit_orders(4):
        both_forms(s, 128, [(parts[0], 150), (parts[1], 150)], v1, v2, ks)
    check_forms(s.run(exe, tmp_path), 2, dropped,
                [cache.get(model.key(af, a)) for af, a in ks], (128, len(cache), 0, 0))
