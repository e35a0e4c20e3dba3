"""What the RX socket demultiplex must give, restated for the tests in pure
Python from the reference: udp_rx builds local = (af, ip->dst, udp->dport) and
remote = (af, ip->src, udp->sport) (udp.c:141-143), asks w_get_sock for the
pair and, if there is none, for the local half alone (udp.c:143-146,
backend_netmap.c:481-490) -- an exact compare of whole tuples
(warpcore.c:644-677), here a dict -- and appends the frame to that socket's
queue in ring order (udp.c:174), or answers unreachable (udp.c:147-155).

It takes frames, the records of rx_deliver_model, and a socket list; nothing
here knows how the library hashes.
"""
from __future__ import annotations

import numpy as np

NONE, UNBOUND, MAX_SOCKS, STARTS = 0xFE, 0xFF, 254, 256

# struct wc_rx_sock, field by field (40 bytes)
SOCK = np.dtype([("af", "u1"), ("connected", "u1"), ("lport", "<u2"), ("rport", "<u2"),
                 ("pad", "<u2"), ("laddr", "u1", 16), ("raddr", "u1", 16)])
assert SOCK.itemsize == 40


def sock(af: int, laddr: bytes, lport: int, raddr: bytes = None, rport: int = 0,
         rng: np.random.Generator = None) -> np.ndarray:
    """One struct wc_rx_sock (a 0-d SOCK array): bound only without `raddr`.
    With `rng`, every byte the library must ignore holds garbage."""
    alen = 4 if af == 4 else 16
    assert len(laddr) == alen and (raddr is None or len(raddr) == alen)
    s = np.zeros((), dtype=SOCK)
    if rng is not None:
        s["pad"] = int(rng.integers(1, 1 << 16))
        s["laddr"] = rng.integers(1, 256, 16, dtype=np.uint8)
        s["raddr"] = rng.integers(1, 256, 16, dtype=np.uint8)
        if raddr is None:
            s["rport"] = int(rng.integers(1, 1 << 16))
    s["af"], s["lport"] = af, lport
    s["laddr"][:alen] = np.frombuffer(laddr, np.uint8)
    if raddr is not None:
        s["connected"], s["rport"] = 1, rport
        s["raddr"][:alen] = np.frombuffer(raddr, np.uint8)
    return s


def sock_tuple(s) -> tuple:
    """The tuple a socket is keyed by: (local, remote), remote None when bound."""
    af = int(s["af"])
    alen = 4 if af == 4 else 16
    local = (af, bytes(s["laddr"][:alen]), int(s["lport"]))
    if not int(s["connected"]):
        return local, None
    return local, (af, bytes(s["raddr"][:alen]), int(s["rport"]))


def valid(socks) -> bool:
    """Whether wc_rx_socktab_build must accept the list."""
    socks = np.asarray(socks, dtype=SOCK).reshape(-1)
    if socks.size > MAX_SOCKS:
        return False
    if any(int(s["af"]) not in (4, 6) or int(s["connected"]) > 1 for s in socks):
        return False
    return len({sock_tuple(s) for s in socks}) == socks.size


class Table:
    """The engine's socket hash (w->b->sock) as a dict."""

    def __init__(self, socks):
        self.socks = np.asarray(socks, dtype=SOCK).reshape(-1)
        assert valid(self.socks)
        self.ns = self.socks.size
        self.map = {sock_tuple(s): i for i, s in enumerate(self.socks)}

    def lookup(self, af: int, laddr: bytes, lport: int, raddr: bytes, rport: int) -> int:
        local = (af, bytes(laddr), lport)
        ws = self.map.get((local, (af, bytes(raddr), rport)))      # udp.c:143
        if ws is None:
            ws = self.map.get((local, None))                      # udp.c:146
        return UNBOUND if ws is None else ws

    def of_frame(self, frame: bytes, rec) -> int:
        """A frame's socket id from its bytes and its record (NONE without one)."""
        af = int(rec["af"])
        if af == 0:
            return NONE
        alen = 4 if af == 4 else 16
        so, do = int(rec["src_off"]), int(rec["dst_off"])
        return self.lookup(af, frame[do:do + alen], int(rec["dport"]),
                           frame[so:so + alen], int(rec["sport"]))


def group(sock_ids: np.ndarray, ns: int):
    """The stable grouped list and start[256] of a socket-id array."""
    ids = np.asarray(sock_ids, dtype=np.uint8)
    runs, start, at = [], np.zeros(STARTS, dtype=np.uint64), 0
    for s in range(ns):
        start[s] = at
        r = np.flatnonzero(ids == s)
        runs.append(r)
        at += r.size
    start[ns:STARTS - 1] = at
    r = np.flatnonzero(ids == UNBOUND)
    runs.append(r)
    start[STARTS - 1] = at + r.size
    return np.concatenate(runs).astype(np.uint32), start


class Expect:
    """A batch's expectation: socket ids, the grouped list and the starts."""

    def __init__(self, table: Table, frames, records):
        self.ns = table.ns
        self.sock = np.array([table.of_frame(bytes(fr)[:flen], records[i])
                              for i, (fr, flen) in enumerate(frames)], dtype=np.uint8) \
            if len(frames) else np.zeros(0, np.uint8)
        self.list, self.start = group(self.sock, self.ns)

    def take(self, idx) -> "Expect":
        """The expectation of the batch whose frame i is this one's frame idx[i]."""
        e = object.__new__(Expect)
        e.ns, e.sock = self.ns, self.sock[idx]
        e.list, e.start = group(e.sock, e.ns)
        return e


def self_check() -> None:
    """The model against hand-worked cases."""
    a, b, c = bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2]), bytes([10, 0, 0, 3])
    t = Table([sock(4, a, 80), sock(4, a, 80, b, 9), sock(6, a + bytes(12), 80)])
    assert t.lookup(4, a, 80, b, 9) == 1          # the connected tuple wins
    assert t.lookup(4, a, 80, b, 10) == 0         # another remote port: the bound one
    assert t.lookup(4, a, 80, c, 9) == 0
    assert t.lookup(4, a, 81, b, 9) == UNBOUND
    assert t.lookup(4, b, 80, b, 9) == UNBOUND
    assert t.lookup(6, a + bytes(12), 80, bytes(16), 1) == 2
    assert t.lookup(6, a + bytes(11) + b"\x01", 80, bytes(16), 1) == UNBOUND
    assert not valid([sock(4, a, 80), sock(4, a, 80)])
    assert not valid([sock(4, a, 80, b, 9), sock(4, a, 80, b, 9)])
    assert valid([sock(4, a, 80, b, 9), sock(4, a, 80, b, 10)])
    bad = sock(4, a, 80)
    bad["af"] = 5
    assert not valid([bad])
    lst, start = group(np.array([1, NONE, 0, UNBOUND, 1, 0, NONE, UNBOUND, 1], np.uint8), 3)
    assert lst.tolist() == [2, 5, 0, 4, 8, 3, 7]
    assert start[:4].tolist() == [0, 2, 5, 5] and (start[3:255] == 5).all() and start[255] == 7
    lst, start = group(np.zeros(0, np.uint8), 0)
    assert lst.size == 0 and not start.any()
