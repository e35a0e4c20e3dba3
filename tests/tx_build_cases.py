"""Inputs of the TX build tests: socket / destination tables, descriptors and
frame layouts (packets.py's scrambled slots and back-to-back packing) whose
every byte -- header area, payload, gaps -- is random before the call."""
from __future__ import annotations

import numpy as np

import tx_build_model as model
from packets import pack, slot_ring

TOS = (0, 1, 2, 3, 0xB8, 0xBB)
DATA_LENS = (0, 1, 2, 7, 8, 15, 16, 17, 31, 33, 63, 64, 65, 127, 129, 1471, 1472, 1473)


def socks_table(rng: np.random.Generator, ns: int) -> np.ndarray:
    """ns sockets cycling through af 4 / 6 x connected x ECN (8 kinds), every
    other byte random -- the ignored ones too."""
    s = np.frombuffer(rng.integers(0, 256, ns * model.SOCK.itemsize, dtype=np.uint8).tobytes(),
                      dtype=model.SOCK).copy()
    k = np.arange(ns)
    s["af"] = np.where(k & 1, 6, 4)
    s["flags"] = (k >> 1) & 3
    return s


def dsts_table(rng: np.random.Generator, nd: int) -> np.ndarray:
    return np.frombuffer(rng.integers(0, 256, nd * model.DST.itemsize, dtype=np.uint8).tobytes(),
                         dtype=model.DST).copy()


def descs_for(rng: np.random.Generator, n: int, ns: int, nd: int, data_lens=None,
              max_len: int = 1472) -> np.ndarray:
    """n descriptors with valid indices (a destination index only where there
    is a table), sockets and TOS values cycling so that every kind meets every
    TOS; lengths from `data_lens` in order, or random up to max_len."""
    d = np.zeros(n, dtype=model.DESC)
    k = np.arange(n)
    d["sock"] = (k + k // max(ns, 1)) % max(ns, 1)
    d["tos"] = np.array(TOS, np.uint8)[(k // 8) % len(TOS)]
    d["dst"] = rng.integers(0, max(nd, 1), n)
    d["ip_id"] = rng.integers(0, 65536, n)
    if data_lens is None:
        d["data_len"] = rng.integers(0, max_len + 1, n)
    else:
        d["data_len"] = np.resize(np.array(data_lens, np.uint16), n)
    return d


def span_of(desc, socks, fallback: int = 60) -> int:
    """Bytes a frame gets in a packed layout: its built length, or `fallback`
    random bytes for a descriptor whose socket index is bad."""
    s = int(desc["sock"])
    if s >= len(socks) or int(socks[s]["af"]) not in (4, 6):
        return fallback
    return model.hdr_len(int(socks[s]["af"])) + int(desc["data_len"])


def lay_out(rng: np.random.Generator, descs, socks, layout: str, slot: int = 2048):
    """(buf, offs, slot_bytes): 'slots' = scrambled `slot`-byte slots, or
    'pack_<align>_<lead>' = back to back; all bytes random."""
    frames = []
    for d in descs:
        ln = min(span_of(d, socks), slot if layout == "slots" else 1 << 20)
        frames.append((bytes(ln), ln))
    if layout == "slots":
        buf, offs, _ = slot_ring(frames, slot=slot, rng=rng)
    else:
        _, align, lead = layout.split("_")
        buf, offs, _ = pack(frames, align=int(align), lead=int(lead))
    buf[:] = rng.integers(0, 256, buf.size, dtype=np.uint8)
    return buf, offs, slot


LAYOUTS = ("slots", "pack_1_0", "pack_1_5", "pack_2_14", "pack_16_3")
