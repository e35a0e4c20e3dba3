"""A deterministic grid of strided batches that stand on, and one chunk above,
every chunk threshold of the strided planner (plan_strided, shape_for_chunks,
lean_shape_for and lean_ph_shape in warpcore_amd/csrc/wc_rt_plan.cpp), for
wc_cksum_strided (ip and payload) and wc_cksum_ip_udp_strided.

A case is (len, stride, base phase, n) plus a byte buffer; packet i of it is
buffer[phase + i * stride : ... + len].  For every threshold T the chunk counts
nch = T and nch = T + 1 are reached

    aligned-exact   phase 0,  len = 16 nch
    tail-masked     phase 0,  len = 16 nch - 1
    head-masked     phase p,  len = 16 nch - p    for p = 1, 2, 14, 15

each at every stride class of STRIDE_CLASSES and every n of N_SET.  Batches
at a stride that is no multiple of 16 are planned for start phase 15 whatever
the base is: there len = 16 nch - 15 stands on the planner's nch, the other
sides one chunk above it.

Every byte of a buffer is random and never 0 -- the bytes before the first
packet, the gaps between packets and the 64 bytes behind the last one
included -- so that a mask that is one byte off changes a sum.  For the
payload and fused kinds the packets' first bytes cycle over HEADER_KINDS, with
the IHL lowered (or IPv6 replaced by IPv4) where len would otherwise be below
the header length: payload_cksum(pkt, len < hl) is outside the reference's
domain.  The one exception is short_header_cases(): IPv4 packets with options
and 20 <= len < hl, for the fused calls' header checksum alone -- ip_cksum(pkt,
hl) is defined whatever len is; the payload value of such a packet is not.

Buffers are built on demand from one seed and the case's own numbers, so the
grid is the same in every process; nothing here needs a GPU.
"""
from __future__ import annotations

import functools
from collections import Counter
from typing import NamedTuple

import numpy as np

from oracle import c_oracle

SEED = 0x57D1D

# --- the planner's chunk thresholds, as they stand in wc_rt_plan.cpp -----------
SHAPE_T = (4, 6, 8, 16, 24, 30, 34, 48, 56, 63, 77, 80, 87, 96, 128, 256, 576)  # shape_for_chunks
SEG_T = (5, 6, 35, 36, 48, 49, 64, 89, 90)   # plan_strided's seg table
SEG_ROWS_T = (5, 9, 14)                      # its 2-row / 4-row choice
LEAN_T = (48, 18)                            # lean_max, the PH path's window
# lean_shape_for takes a packet whose chunks fill one pass exactly: 8, 16, 24,
# 32 and 48 chunks below lean_max.  32 is the one that no other table names.
LEAN_FILL_T = (8, 16, 24, 32, 48)
THRESHOLDS = tuple(sorted(set(SHAPE_T + SEG_T + SEG_ROWS_T + LEAN_T + LEAN_FILL_T)))
LEAN_PAYLOAD_LENS = (47, 48, 49)             # payload_cksum's len >= 48 on the lean kernel
EXTRA_LENS = (65535, 9000, 1, 0)             # (0: ip only)

PHASES = (0, 1, 2, 14, 15)
# (mask side, base phase, bytes that len is short of 16 * nch)
SIDES = (("exact", 0, 0), ("tail", 0, 1), ("head", 1, 1), ("head", 2, 2), ("head", 14, 14),
         ("head", 15, 15))
STRIDE_CLASSES = ("len", "len+1", "len+len/8", "len+len/8+1", "mult16", "mult64", "sparse-16",
                  "sparse", "slot")
N_SET = (1, 63, 64, 151)   # no seg route (n < 64) | the first n with it | a tail wave for
N_LONG = (1, 63, 64, 67)   # every PPW of 2..64 (odd); fewer packets above LONG bytes
N_HUGE = (1, 3)            # 65535 B: no seg route at any n, one packet per wave
LONG = 2100
TAIL = 64                  # random bytes behind the last packet

KINDS = ("ip", "payload", "fused")
HEADER_KINDS = ("v4-ihl5", "v4-options", "v4-ihl<5", "v6-udp", "v6-nh254/255", "random")


class Case(NamedTuple):
    length: int
    stride: int
    phase: int
    n: int
    cells: tuple   # ((threshold, "at" | "above", side, phase, stride class), ...)
    kinds: tuple   # of KINDS

    @property
    def group(self):
        """The cases that share a buffer: the same but for n."""
        return self.length, self.stride, self.phase

    @property
    def offs(self) -> np.ndarray:
        return np.arange(self.n, dtype=np.uint64) * np.uint64(self.stride) + np.uint64(self.phase)


def chunks(length: int, phase: int, payload: bool = False) -> int:
    """The 16-byte chunks a packet touches (payload_cksum reads 20 bytes)."""
    return (phase + (max(length, 20) if payload else length) + 15) // 16


def strides_for(length: int, nch: int) -> dict:
    """stride -> the classes it stands for, for a packet of `nch` chunks."""
    up = lambda v, m: max(m, (v + m - 1) // m * m)  # noqa: E731
    sparse = up(32 * nch, 16)
    vals = (("len", length), ("len+1", length + 1), ("len+len/8", length + length // 8),
            ("len+len/8+1", length + length // 8 + 1), ("mult16", up(length, 16)),
            ("mult64", up(length, 64)), ("sparse-16", max(sparse - 16, length)),
            ("sparse", sparse), ("slot", up(length + 16, 2048)))
    out: dict = {}
    for name, v in vals:
        out.setdefault(v, []).append(name)
    return out


def _n_set(length: int) -> tuple:
    return N_HUGE if length > 60000 else N_LONG if length > LONG else N_SET


@functools.lru_cache(maxsize=None)
def grid() -> tuple:
    """Every case, each (len, stride, phase, n) once, with the census cells
    it stands in."""
    cells: dict = {}

    def add(length, phase, nch, label, where, side):
        for stride, classes in strides_for(length, nch).items():
            for n in _n_set(length):
                key = (length, stride, phase, n)
                cells.setdefault(key, []).extend((label, where, side, phase, c) for c in classes)

    for t in THRESHOLDS:
        for where, nch in (("at", t), ("above", t + 1)):
            for side, phase, short in SIDES:
                add(16 * nch - short, phase, nch, t, where, side)
    for length in LEAN_PAYLOAD_LENS + EXTRA_LENS:
        label = "len48" if length in LEAN_PAYLOAD_LENS else "extra"
        for phase in PHASES:
            add(length, phase, chunks(length, phase), label, str(length), "any")
    return tuple(Case(*key, tuple(c), KINDS if key[0] else ("ip",)) for key, c in cells.items())


def census(cases) -> Counter:
    """Cases per (threshold, at | above, mask side, phase, stride class)."""
    c: Counter = Counter()
    for case in cases:
        c.update(case.cells)
    return c


def expected_cells() -> set:
    out = {(t, where, side, phase, cls) for t in THRESHOLDS for where in ("at", "above")
           for side, phase, _ in SIDES for cls in STRIDE_CLASSES}
    for length in LEAN_PAYLOAD_LENS + EXTRA_LENS:
        label = "len48" if length in LEAN_PAYLOAD_LENS else "extra"
        out |= {(label, str(length), "any", p, cls) for p in PHASES for cls in STRIDE_CLASSES}
    return out


def for_threshold(label) -> tuple:
    """The cases standing at threshold `label` (or "len48" / "extra")."""
    return tuple(c for c in grid() if any(cell[0] == label for cell in c.cells))


LABELS = THRESHOLDS + ("len48", "extra")


# --- buffers --------------------------------------------------------------------

def hdr_len(first) -> np.ndarray:
    """4 * IHL where the version nibble is 4, else 40 (in_cksum.c:149-160)."""
    b = np.asarray(first).astype(np.int64)
    return np.where(b >> 4 == 4, (b & 0x0F) * 4, 40)


def _be16(buf, at, v):
    buf[at] = v >> 8
    buf[at + 1] = v & 0xFF


def _max_n(group) -> int:
    return _n_set(group[0])[-1]


def header_kind(i: int, rot: int) -> int:
    return (i + rot) % len(HEADER_KINDS)


def _plant_headers(buf, length, stride, phase, n, rng) -> None:
    """First bytes of the packets, cycling over HEADER_KINDS; len >= hl kept."""
    rot = (length + stride + phase) % len(HEADER_KINDS)
    most = length // 4  # the largest IHL with hl <= len
    for i in range(n):
        o = phase + i * stride
        kind, j = header_kind(i, rot), i // len(HEADER_KINDS)
        if kind in (3, 4) and length >= 40:
            buf[o] = 0x60
            _be16(buf, o + 4, length - 40)
            buf[o + 6] = 17 if kind == 3 else 254 + j % 2
            continue
        if kind == 5:
            first = int(rng.integers(0, 256))
            if int(hdr_len(first)) <= length:
                buf[o] = first
                continue
            ihl = first & 0x0F
        else:
            ihl = {0: 5, 1: 6 + j % 10, 2: j % 5}.get(kind, 5)
        buf[o] = 0x40 | min(ihl, most)
        if kind == 0 and length >= 20:  # well-formed: total length, DF, UDP
            _be16(buf, o + 2, length)
            _be16(buf, o + 6, 0x4000)
            buf[o + 9] = 17


@functools.lru_cache(maxsize=64)
def _group_buffer(group) -> np.ndarray:
    length, stride, phase = group
    n = _max_n(group)
    rng = np.random.default_rng([SEED, length, stride, phase])
    buf = rng.integers(1, 256, phase + (n - 1) * stride + max(length, 20) + TAIL, dtype=np.uint8)
    if length:
        _plant_headers(buf, length, stride, phase, n, rng)
    buf.setflags(write=False)
    return buf


def buffer(case) -> np.ndarray:
    """The case's bytes (read-only; shared by the cases of its group, whose
    smaller n are prefixes of the largest)."""
    return _group_buffer(case.group)


def header_checksums(buf, offs) -> np.ndarray:
    """ip_cksum(pkt, ip4_hl(pkt[0])) of each IPv4 packet, 0 for any other
    version: what wc_cksum.h defines for d_out_ip_hdr."""
    first = buf[offs.astype(np.int64)]
    v4 = first >> 4 == 4
    hl = np.where(v4, (first & 0x0F).astype(np.uint16) * 4, 0).astype(np.uint16)
    return np.where(v4, c_oracle.cksum_ragged(buf, offs, hl, kind=0), 0).astype(np.uint16)


@functools.lru_cache(maxsize=64)
def _group_expect(group, kinds) -> dict:
    length, stride, phase = group
    n = _max_n(group)
    buf = _group_buffer(group)
    out = {"ip": c_oracle.cksum_strided(buf, stride, length, n, kind=0, byte_offset=phase)}
    if "payload" in kinds:
        out["payload"] = c_oracle.cksum_strided(buf, stride, length, n, kind=1, byte_offset=phase)
        offs = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(phase)
        out["hdr"] = header_checksums(buf, offs)
    return out


def expect(case) -> dict:
    """{"ip", "payload", "hdr"} -> uint16[n] by the C oracle ("ip" alone for a
    case without the payload kinds)."""
    return {k: v[:case.n] for k, v in _group_expect(case.group, case.kinds).items()}


def groups(cases) -> list:
    """One case per buffer: the one with the largest n."""
    best: dict = {}
    for c in cases:
        if c.group not in best or c.n > best[c.group].n:
            best[c.group] = c
    return list(best.values())


# --- IPv4 headers longer than len -------------------------------------------------

SHORT_LENS = (20, 23, 24, 31, 32, 36, 47, 48, 59)   # 20 <= len < 60
SHORT_STRIDES = ("packed", 64, 2048)


class ShortCase(NamedTuple):
    length: int
    stride: int
    phase: int
    n: int

    @property
    def offs(self) -> np.ndarray:
        return np.arange(self.n, dtype=np.uint64) * np.uint64(self.stride) + np.uint64(self.phase)


@functools.lru_cache(maxsize=None)
def short_header_cases() -> tuple:
    return tuple(ShortCase(length, length if stride == "packed" else stride, phase, n)
                 for length in SHORT_LENS for stride in SHORT_STRIDES for phase in PHASES
                 for n in N_SET)


def short_ihl(length: int, i: int) -> int:
    """IHL of packet i: cycling over 6..15 where 4 * IHL > len."""
    lo = max(6, length // 4 + 1)
    return lo + i % (16 - lo)


@functools.lru_cache(maxsize=64)
def _short_buffer(length, stride, phase) -> np.ndarray:
    n = N_SET[-1]
    rng = np.random.default_rng([SEED, 0x5407, length, stride, phase])
    buf = rng.integers(1, 256, phase + (n - 1) * stride + 60 + TAIL, dtype=np.uint8)
    for i in range(n):
        buf[phase + i * stride] = 0x40 | short_ihl(length, i)
    buf.setflags(write=False)
    return buf


def short_buffer(case) -> np.ndarray:
    """The whole header of every packet lies inside it, at any stride (at the
    packed one the headers overlap the packets behind them)."""
    return _short_buffer(case.length, case.stride, case.phase)


def short_expect(case) -> np.ndarray:
    """The header checksums alone: the payload value is unspecified here."""
    return header_checksums(short_buffer(case), case.offs)


@functools.lru_cache(maxsize=None)
def short_packets() -> tuple:
    """The same family as (bytes, len) packets for packets.pack: every IHL
    6..15 x every SHORT_LENS below its header, the bytes being the whole
    header; repeated so that a layout has several 64-packet tiles."""
    rng = np.random.default_rng([SEED, 0x5408])
    out = []
    for rep in range(12):
        for ihl in range(6, 16):
            for length in SHORT_LENS:
                if length >= 4 * ihl:
                    continue
                b = bytearray(rng.integers(1, 256, 4 * ihl, dtype=np.uint8).tobytes())
                b[0] = 0x40 | ihl
                out.append((bytes(b), length))
    return tuple(out)
