"""Worlds for the TX pump tests, composed from the TX neighbour and TX build
cases: a neighbour cache (with a cached broadcast MAC), a destination table
drawn from it and from a small pool of unknown addresses (repeats, both
families, d_af values of 0 and 7), tx_neigh_cases' five sockets (connected and
not, both families, a bad family), descriptors whose socket index lies inside,
at and past the socket table and whose destination index lies inside, at and
past the destination table -- so that a destination's family is often not the
socket's --, payloads of tx_build_cases.DATA_LENS plus frames longer than the
slot and longer than any frame, in tx_build_cases' layouts, and solicitation
slots as rx_reply_cases lays them out."""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

import rx_reply_cases as rc
import tx_build_cases as bc
import tx_neigh_cases as nc
import tx_neigh_model as nmodel
import tx_pump_model as model

SMALL, SMALL_DST = model.SMALL, model.SMALL_DST
SLOT, SOL_SLOT = 2048, 128
LAYOUTS = ("slots", "pack_1_5")  # of tx_build_cases.LAYOUTS
assert set(LAYOUTS) <= set(bc.LAYOUTS) and {0, 1472} <= set(bc.DATA_LENS)
CENSUS = (600, 257)


def cache_of(known, seed: int, bcast_every: int = 9) -> dict:
    """A MAC for every known key; every bcast_every-th one is ff x 6 (cached,
    and still unresolved: neighbor.c:102)."""
    rng = np.random.default_rng(seed)
    return {nmodel.key(af, a): (nmodel.BCAST if bcast_every and i % bcast_every == 4 else nc.mac_of(rng))
            for i, (af, a) in enumerate(known)}


def records_of(cache: dict) -> np.ndarray:
    """The cache as update records, for wc_neigh_apply."""
    return nmodel.records([(af, mac, a) for (af, a), mac in cache.items()])


def descs_of(seed: int, n: int, ns: int, ndst: int, connected_only: bool = False) -> np.ndarray:
    """hold_world's walk through the chain's branches, two thirds of it re-drawn
    over this world's tables; lengths from DATA_LENS, some past the slot, some
    past 65535 - headers."""
    rng = np.random.default_rng(seed)
    d = nc.hold_world(n, seed)
    k = np.arange(n)
    redraw = rng.random(n) < 0.67
    d["sock"] = np.where(redraw, rng.integers(0, 4, n), d["sock"])
    at = rng.random(n)
    dst = np.where(at < 0.05, ndst, np.where(at < 0.08, 65535, rng.integers(0, max(ndst, 1), n)))
    d["dst"] = np.where(redraw, dst, d["dst"])
    d["sock"] = np.where(k % 41 == 7, ns, d["sock"])  # at the table's end
    if connected_only:
        d["sock"] = 2 + (k & 1)
    d["tos"] = np.array(bc.TOS, np.uint8)[(k // 8) % len(bc.TOS)]
    d["ip_id"] = rng.integers(0, 65536, n)
    lens = np.resize(np.array(bc.DATA_LENS, np.uint16), n)
    lens[rng.permutation(n)[:n // 2]] = rng.integers(0, 200, n // 2)
    lens[k % 13 == 5] = 3000    # longer than the slot
    lens[k % 29 == 11] = 65535  # longer than a frame can be
    d["data_len"] = lens
    return d


def world(seed: int, n: int, ndst: int, layout: str = "slots", hit: float = 0.5, m: int = None,
          nknown: int = 40, connected_only: bool = False, engine=None):
    """One batch: every input of wc_tx_pump on the host.  m: the solicitation
    slots (default: a few more than can be asked for)."""
    rng = np.random.default_rng(seed)
    w = SimpleNamespace(seed=seed, n=n, ndst=ndst, layout=layout)
    w.known = nc.keys(nknown, rng)
    w.cache = cache_of(w.known, seed)
    w.dsts, w.afs = nc.dst_world(seed, ndst, w.known, hit)
    if ndst >= 16:  # d_af values of 0 and 7, wherever the draw put none
        w.afs[5::max(16, ndst // 12)] = 0
        w.afs[9::max(16, ndst // 12)] = 7
    w.socks = nc.socks_table()
    w.descs = descs_of(seed, n, len(w.socks), ndst, connected_only)
    if n:
        room = w.descs.copy()  # a frame too long to exist is never built or read: 60 bytes do
        room["data_len"][room["data_len"] > 65000] = 18
        w.buf, w.offs, w.slot = bc.lay_out(rng, room, w.socks, layout, SLOT)
    else:  # no frame: bytes that must stay what they are
        w.buf, w.offs, w.slot = rng.integers(0, 256, 64, dtype=np.uint8), [], SLOT
    w.offs = np.asarray(w.offs, np.uint64)
    w.eng = rc.engine_table(rng=np.random.default_rng(seed)) if engine is None else engine
    w.m = ndst + 3 if m is None else m
    w.sol, w.sol_offs = rc.out_slots(w.m, SOL_SLOT, rng)
    w.sol_offs = np.asarray(w.sol_offs, np.uint64)
    return w


def expect(w, zero_udp: bool = False):
    return model.expect(w.cache, w.dsts, w.afs, w.descs, w.socks, w.buf, w.offs, w.slot, zero_udp,
                        w.eng, w.sol, w.sol_offs, SOL_SLOT)
