"""What the RX echo must give, restated for the tests in numpy from wc_cksum.h
("RX echo"): which frames are echoed and in which order, each entry's status,
descriptor, destination, family, source index and offset, and where its payload
goes.  It works from frames, the records of rx_deliver_model, the list / start
of rx_demux_model and a map; nothing here knows how the kernel finds an entry.
"""
from __future__ import annotations

from types import SimpleNamespace

import numpy as np

from rx_deliver_model import RECORD
from tx_build_model import DESC, DST

ECHO, NONE, SHORT, NO_ROOM, STALE = 0, 4, 8, 9, 10
OFF, MAX, MAX_SOCKS = 0xFFFF, 65536, 254
NO_FRAME = 0xFFFFFFFF
SKIPPED = (SHORT, NO_ROOM, STALE)


def hl_tx(af: int) -> int:
    return 20 if af == 4 else 40


def run_lengths(start, emap, n: int) -> list:
    """The length of every socket's run under the clamp rule: 0 for a socket
    that is off, and unless start[s] <= start[s + 1] <= n."""
    out = []
    for s in range(len(emap)):
        s0, s1 = int(start[s]), int(start[s + 1])
        out.append(s1 - s0 if int(emap[s]) <= 255 and s0 <= s1 <= n else 0)
    return out


def order(start, emap, n: int) -> list:
    """[(socket, list position)] of every echo entry, in echo order."""
    return [(s, int(start[s]) + k) for s, ln in enumerate(run_lengths(start, emap, n))
            for k in range(ln)]


def status_of(i: int, n: int, rec, flen: int, copy: bool, out_slot_bytes: int) -> int:
    """The first rule that holds names the status (wc_cksum.h)."""
    if i >= n:
        return STALE
    af, hl = int(rec["af"]), int(rec["hl"])
    if af not in (4, 6):
        return STALE
    if hl < hl_tx(af) or int(rec["data_off"]) != 14 + hl + 8 \
            or int(rec["src_off"]) + (4 if af == 4 else 16) > flen:
        return STALE
    if int(rec["data_off"]) + int(rec["data_len"]) > flen:
        return SHORT
    if copy and 14 + hl_tx(af) + 8 + int(rec["data_len"]) > out_slot_bytes:
        return NO_ROOM
    return ECHO


def echo(buf: np.ndarray, offs, lens, rec, lst, start, emap, m: int, copy: bool,
         out_slot_bytes: int = 2048, ip_ids=None, n=None):
    """Every output of wc_rx_echo for m entries.  payload[j]: the bytes copy
    mode puts at slot j + 14 + hl_tx + 8 (None: nothing is copied); in in-place
    mode the same bytes are what already lies behind tx_off[j]'s header space."""
    n = len(offs) if n is None else n
    rec = np.asarray(rec).view(RECORD).reshape(-1)
    ents = order(start, emap, n) if n and len(emap) else []
    o = SimpleNamespace(E=len(ents), desc=np.zeros(m, DESC), dsts=np.zeros(m, DST),
                        af=np.zeros(m, np.uint8), status=np.full(m, NONE, np.uint8),
                        src=np.full(m, NO_FRAME, np.uint32), tx_off=np.zeros(m, np.uint64),
                        payload=[None] * m, sock=[None] * m)
    o.desc["data_len"], o.desc["dst"] = 0xFFFF, np.arange(m)
    for j, (s, at) in enumerate(ents[:m]):
        i = int(lst[at])
        r = rec[i] if i < n else None
        flen = int(lens[i]) if i < n else 0
        st = status_of(i, n, r, flen, copy, out_slot_bytes)
        o.status[j], o.sock[j] = st, s
        if i < n:
            o.src[j] = i
        if st != ECHO:
            continue
        af, base = int(r["af"]), int(offs[i])
        fr = buf[base:base + flen]
        o.desc[j] = (int(r["data_len"]), 0 if ip_ids is None else int(ip_ids[j]),
                     int(emap[s]) & 0xFF, int(r["tos"]), j)
        so, alen = int(r["src_off"]), 4 if af == 4 else 16
        o.dsts[j]["addr"][:alen] = fr[so:so + alen]
        o.dsts[j]["dmac"] = fr[6:12]
        o.dsts[j]["port"] = int(r["sport"])
        o.af[j] = af
        do = int(r["data_off"])
        o.payload[j] = fr[do:do + int(r["data_len"])].tobytes()
        if not copy:
            o.tx_off[j] = base + int(r["hl"]) - hl_tx(af)
    o.skipped = int(np.isin(o.status, SKIPPED).sum())
    return o
