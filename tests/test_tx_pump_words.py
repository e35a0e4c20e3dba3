"""CPU test of the lines the TX pump's kernels compile
(warpcore_amd/csrc/wc_tx_pump.h), compiled for the host alone
(tests/c/tx_pump_words.cpp, with -fsanitize=address,undefined, run directly):
the per-frame gate over the full grid of hold codes x check-chain outcomes x
flag, and the plan launch's destination steps -- find, a barrier, mark -- with
the destinations visited in order, reversed and shuffled between the barriers;
all against tests/tx_pump_model.py and tests/tx_neigh_model.py."""
import itertools
import struct
import subprocess

import numpy as np
import pytest

import cprog
import tx_build_model as bmodel
import tx_neigh_cases as nc
import tx_neigh_model as nmodel
import tx_pump_model as model


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return cprog.build_words("tx_pump_words", tmp_path_factory.mktemp("txp"))


def run(exe, tmp_path, blob: bytes) -> bytes:
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(blob)
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return dst.read_bytes()


def test_gate_over_the_full_grid(exe, tmp_path):
    """Every hold code (and bytes that are none) x every outcome of the build's
    check chain x the flag.  The chain's own status is held against
    tx_build_model.status_of on a one-socket, one-destination world."""
    holds = (nmodel.TH_READY, nmodel.TH_MALFORMED, nmodel.TH_HELD, 1, 0x80, 0xFF)
    afs, flags = (4, 6, 0, 9), (0, 1, 2, 3)
    lens = (0, 1, 1472, 1986, 1987, 2006, 2007, 3000, 65473, 65474, 65493, 65494, 65535)
    grid = list(itertools.product(holds, (0, 1), afs, flags, (0, 1), lens, (2048, 65535), (0, 1)))
    blob = struct.pack("<2I", 3, len(grid))
    for hold, sock_in, af, fl, dst_in, dl, slot, zero in grid:
        blob += struct.pack("<7I", hold, sock_in, af | fl << 8 | 0x1234 << 16, dst_in, dl, slot, zero)
    got = np.frombuffer(run(exe, tmp_path, blob), "<u4").reshape(len(grid), 6)
    seen = set()
    for row, (hold, sock_in, af, fl, dst_in, dl, slot, zero) in zip(got, grid):
        socks = np.zeros(1, bmodel.SOCK)
        socks["af"], socks["flags"] = af, fl
        desc = np.zeros(1, bmodel.DESC)[0]
        desc["sock"], desc["dst"], desc["data_len"] = 0 if sock_in else 1, 0 if dst_in else 1, dl
        st = bmodel.status_of(desc, socks, 1, slot, bool(zero))
        assert row[0] == st, (hold, sock_in, af, fl, dst_in, dl, slot, zero)
        flen = bmodel.hdr_len(af) + dl
        want = model.gate(hold if hold in (0, 4, 8) else nmodel.TH_MALFORMED, st, flen)
        assert tuple(row[2:]) == tuple(int(x) for x in want), (hold, st, row)
        if af in (4, 6):
            assert row[1] == flen
        seen.add((hold, st))
    assert seen >= set(itertools.product(holds, (0, 1, 6, 7)))


def orders(n: int, k: int = 6, seed: int = 1):
    rng = np.random.default_rng(seed)
    ident = np.arange(n, dtype=np.uint32)
    out = [(ident, ident), (ident[::-1], ident[::-1]), (ident, ident[::-1]), (ident[::-1], ident)]
    return out + [(rng.permutation(n).astype(np.uint32), rng.permutation(n).astype(np.uint32))
                  for _ in range(k)]


def test_destination_steps_in_any_order(exe, tmp_path):
    """80 destinations, 9 distinct unresolved addresses (one of them a cached
    broadcast MAC), bad families in between: state and dmac are the model's in
    every order."""
    rng = np.random.default_rng(5)
    known = nc.keys(12, rng)
    cache = {nmodel.key(af, a): nc.mac_of(rng) for af, a in known}
    cache[nmodel.key(*known[3])] = nmodel.BCAST
    unknown = [(4, nc.addr4(30000 + i) + bytes(12)) for i in range(4)] + \
        [(6, nc.addr6(31000 + i)) for i in range(4)] + [known[3]]
    picks = [unknown[(i * 7) % 9] if i % 4 else known[int(rng.integers(0, 12))] for i in range(80)]
    afs = np.array([af for af, _ in picks], np.uint8)
    afs[[7, 33, 70]] = (0, 7, 255)
    dsts = nc.dst_table([(a, 4433 + i) for i, (_, a) in enumerate(picks)], rng)
    state, after, miss = nmodel.resolve(cache, dsts, afs)
    distinct = {nmodel.key(int(afs[k]), bytes(dsts["addr"][k])) for k in range(80)
                if state[k] in (nmodel.MISS, nmodel.MISS_DUP)}
    assert len(distinct) == 9 == len(miss) and (state == nmodel.MISS_DUP).sum() > 20
    upd = nmodel.records([(af, mac, a) for (af, a), mac in cache.items()])
    head = struct.pack("<2I", 1, 64) + struct.pack("<2I", 2, upd.size) + upd.tobytes()
    body = struct.pack("<2I", 4, 80) + dsts.tobytes() + afs.tobytes()
    for o1, o2 in orders(80):
        raw = run(exe, tmp_path, head + body + o1.tobytes() + o2.tobytes())
        assert struct.unpack("<I", raw[:4])[0] == 0
        got_state = np.frombuffer(raw[4:84], np.uint8)
        got_dsts = np.frombuffer(raw[84:], nmodel.DST)
        assert (got_state == state).all(), (o1[:8], np.flatnonzero(got_state != state))
        assert got_dsts.tobytes() == after.tobytes()
