"""Worlds for the RX answer tests: rx_drain_cases' mixed ring (the frames of
rx_demux_cases, rx_reply_cases.world and rx_neigh_cases.world), plus the frames
the generators alone do not reach -- rx_neigh_cases.peer_requests and, in both
families, addresses that several ARP frames / neighbour solicitations name with
different MACs, so that "the last record wins" is exercised by the ring itself.

answer() states every output of wc_rx_answer from the models alone:
rx_reply_model's built frames, rx_neigh_model's built frames and update records
and tx_neigh_model.apply for the cache.  The answer's slot_bytes (SLOT) is
smaller than the plan's (rx_drain_cases.WORLDS), so some listed echoes find no
room at build time: length 0, slot untouched."""
from __future__ import annotations

import copy
from types import SimpleNamespace

import numpy as np

import rx_drain_cases as dcases
import rx_neigh_cases as nc
import rx_neigh_model as nmodel
import rx_reply_cases as rc
import rx_reply_model as rmodel
import tx_neigh_model as tmodel

SMALL = 4096  # WC_RX_ANSWER_SMALL
N = 600
SLOT = 128    # the answer's slot_bytes: an advertisement (86) fits, a long echo does not
REPEATS = 10  # addresses per family named twice or three times with different MACs
# layout -> (seed, frames, sockets, the plan's slot_bytes): seeds at which the
# 600 frames meet every condition of test_rx_answer_model.py
WORLDS = {"slots": (3, N, 6, 256), "packed": (15, N, 6, 256)}


def repeated_keys(rng):
    """ARP replies / requests and neighbour solicitations for us from REPEATS
    hosts per family, each host two or three times with another MAC."""
    out = []
    for k in range(REPEATS):
        a4 = bytes((192, 168, 77, 1 + k))
        a6 = nc.PEER6[:8] + bytes((0x77, 0, 0, 0, 0, 0, 0, 1 + k))
        for rep in range(2 + k % 2):
            mac = bytes((2, 0, 0, 7, rep, int(rng.integers(0, 256))))
            if (k + rep) % 2:
                out.append(nc.arp(op=b"\x00\x02", sha=mac, spa=a4, tha=rc.MAC, dst=rc.MAC))
            else:
                out.append(nc.arp(tpa=nc.A4[k % 2], sha=mac, spa=a4))
            out.append(nc.nd(135, nc.A6[k % 2], opt=b"\x01\x01" + mac, src=a6))
    return out


def world(seed: int, n: int = N, ns: int = 6):
    """(frames, socks): n frames, the extra ones at seeded places of the ring."""
    rng = np.random.default_rng(seed + 100)
    extra = [f[0] for f in nc.peer_requests()] + repeated_keys(rng)
    frames, socks = dcases.world(seed, n - len(extra), ns)
    for fr in extra:
        frames.insert(int(rng.integers(0, len(frames) + 1)), fr)
    return frames, socks


def subset(ex, idx):
    """The reply and neighbour expectations (rx_drain_cases.expect's .reply and
    .neigh) of the batch whose frame i is the base world's frame idx[i]."""
    idx = np.asarray(idx)
    r = object.__new__(rmodel.Expect)
    r.frames = [ex.reply.frames[int(i)] for i in idx]
    r.eng, r.slot_bytes = ex.reply.eng, ex.reply.slot_bytes
    r.action, r.reply_len = ex.reply.action[idx], ex.reply.reply_len[idx]
    r.list = np.flatnonzero((rmodel.MASK_REPLY >> r.action.astype(np.uint32)) & 1).astype(np.uint32)
    nb = object.__new__(nmodel.Expect)
    nb.frames, nb.eng = r.frames, ex.neigh.eng
    nb.nact = ex.neigh.nact[idx]
    nb.why = [ex.neigh.why[int(i)] for i in idx]
    bits = nb.nact.astype(np.uint32)
    nb.rlist = np.flatnonzero((nmodel.MASK_REPLY >> bits) & 1).astype(np.uint32)
    nb.ulist = np.flatnonzero((nmodel.MASK_UPDATE >> bits) & 1).astype(np.uint32)
    return SimpleNamespace(reply=r, neigh=nb)


def answer(ex, r_out0, r_offs, n_out0, n_offs, u_m: int, slot: int = SLOT, ip_ids=None,
           cache: dict = None, cap: int = None):
    """Every output of wc_rx_answer over ex (.reply, .neigh) from the models:
    both output buffers, both length arrays, both built counts, the u_m records
    and -- with `cache`, which is updated -- the number of records dropped."""
    reply = copy.copy(ex.reply)
    reply.slot_bytes = slot
    r_out, r_len, r_built = reply.built(r_out0, r_offs, ip_ids)
    n_out, n_len, n_built = ex.neigh.built(n_out0, n_offs, slot)
    upd = ex.neigh.updates(u_m)
    dropped = 0
    if cache is not None and u_m:
        dropped = tmodel.apply(cache, upd, len(ex.neigh.ulist), u_m, cap)
    return SimpleNamespace(r_out=r_out, r_len=r_len, r_built=r_built, n_out=n_out, n_len=n_len,
                           n_built=n_built, upd=upd, dropped=dropped)


def refused(ex, slot: int = SLOT):
    """The listed replies the build refuses at `slot`: [(list entry, frame)]."""
    out = []
    for j, i in enumerate(ex.reply.list.tolist()):
        r = rmodel.build(ex.reply.frames[i], int(ex.reply.action[i]), ex.reply.eng)
        if r is None or len(r) > slot:
            out.append((j, i))
    return out


def contested(upd: np.ndarray, count: int):
    """{af: the keys two or more of the first `count` records name with
    different MACs}."""
    macs = {}
    u = upd.reshape(-1).view(tmodel.UPDATE).reshape(-1)
    for j in range(count):
        af = int(u["af"][j])
        if af in (4, 6):
            macs.setdefault(tmodel.key(af, bytes(u["addr"][j])), set()).add(bytes(u["mac"][j]))
    out = {4: [], 6: []}
    for k, s in macs.items():
        if len(s) >= 2:
            out[k[0]].append(k)
    return out
