"""A deterministic grid of frames that sit on, one below and one above every
threshold of the per-frame decision chains (rx_decide behind frame_hdr and
frame_hdr_slow, sv_rx, tx_decide, rx_record):

    flen < 14 | room < max(hl, 20) | ip_plen < 8 | room < hl + 8 |
    min(ulen, ip_plen) | room < udp_len + hl | udp_len < 8 (the seal) |
    (udp_len - 8) & 0xFFFF (the record)

grid() returns (frame_bytes, flen, tag) triples.  Bytes of frame_bytes past
flen are not part of the frame and are adversarial on purpose: in a cut frame
they are the frame's true continuation, so a parse that reads them answers OK
where the reference's reads leave the frame (TRUNCATED).  Frames are built
with the builders of packets.py from one seed; nothing here needs a GPU.

census() counts, per decision, the frames at threshold - 1, threshold and
threshold + 1 by header shape and by the verdict they got: the proof that the
grid stands where it claims to.
"""
from __future__ import annotations

import functools
from collections import Counter

import numpy as np

from oracle import c_oracle, py_oracle
from packets import eth_frame, finish_udp, ipv4_udp, ipv6_udp, pack

SEED = 0x0ED6E5
MAX_FRAME = 128          # every frame_bytes is shorter: one 128-byte slot holds it
SHAPES = tuple(range(5, 16)) + (6 * 16,)  # IPv4 IHL 5..15, and IPv6 (named 96 = 0x60)
LADDER_BASES = (5, 11, 96)                # one-round parse, two-round parse, IPv6
V6 = 96

OK, OK_NO_CKSUM, BAD_IP, BAD_UDP, SHORT, FRAGMENT, BAD_VERSION, NOT_UDP, NOT_IP, TRUNCATED = \
    range(10)


def shape_name(shape: int) -> str:
    return "v6" if shape == V6 else f"ihl{shape}"


def _be16(v: int) -> bytes:
    return bytes(((v >> 8) & 0xFF, v & 0xFF))


def _le16(v: int) -> bytes:
    return bytes((v & 0xFF, v >> 8))


def _rand(rng, n: int) -> bytes:
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _ip_packet(shape: int, payload: bytes, rng) -> bytes:
    return ipv6_udp(payload, rng)[0] if shape == V6 else ipv4_udp(payload, rng, ihl=shape)[0]


def _etype(shape: int) -> int:
    return 0x86DD if shape == V6 else 0x0800


def fix_ip4_cksum(ip: bytearray) -> None:
    """Redo the IPv4 header checksum so that ip_cksum(ip, hl) == 0: in its own
    field where that lies inside the summed bytes (hl >= 12), in the id word
    for hl 8; for hl 0 and 4 no word of the sum is free."""
    hl = (ip[0] & 0x0F) * 4
    at = 10 if hl >= 12 else 4 if hl == 8 else None
    if at is None or len(ip) < max(hl, 12):
        return
    ip[at:at + 2] = b"\x00\x00"
    ip[at:at + 2] = _le16(py_oracle.ip_cksum(bytes(ip[:hl])))


def _fields(ip: bytes, v4: bool):
    hl = (ip[0] & 0x0F) * 4 if v4 else 40
    ip_plen = ((((ip[2] << 8) | ip[3]) - hl) & 0xFFFF) if v4 else (ip[4] << 8) | ip[5]
    return hl, ip_plen


def pass_udp(ip: bytearray, v4: bool) -> bool:
    """Make payload_cksum(ip, min(ulen, ip_plen) + hl) come out 0 with a
    non-zero udp->cksum, all of `ip` being inside the frame: the complement
    goes into the field where the summed range holds it (udp_len >= 8), into
    the source-port word for 2 <= udp_len < 8, into an address word (and the
    header checksum redone) below that.  False, the packet unchanged but for
    a non-zero field, where the range runs past `ip`."""
    hl, ip_plen = _fields(ip, v4)
    if len(ip) < hl + 8:
        return False
    udp_len = min((ip[hl + 4] << 8) | ip[hl + 5], ip_plen)
    plen = hl + udp_len
    at = hl + 6 if udp_len >= 8 else hl if udp_len >= 2 else 12 if v4 else 8
    if at != hl + 6 or plen > len(ip):
        ip[hl + 6:hl + 8] = b"\xa5\x5a"  # odd-length ranges end on its first byte
    if plen > len(ip):
        return False
    ip[at:at + 2] = b"\x00\x00"
    ip[at:at + 2] = _le16(py_oracle.payload_cksum(bytes(ip), plen))
    if at == 12:
        fix_ip4_cksum(ip)
    return True


class _Grid:
    def __init__(self):
        self.rng = np.random.default_rng(SEED)
        self.out: list[tuple[bytes, int, str]] = []

    def add(self, frame: bytes, flen: int, tag: str) -> None:
        assert 0 <= flen <= len(frame) < MAX_FRAME, (tag, flen, len(frame))
        self.out.append((bytes(frame), flen, tag))

    def frame(self, shape: int, ip: bytes, etype=None) -> bytes:
        return eth_frame(bytes(ip), self.rng, _etype(shape) if etype is None else etype)

    # --- a. cut ladder -------------------------------------------------------

    def cut_ladder(self) -> None:
        rng = self.rng
        for shape in SHAPES:
            name = shape_name(shape)
            for plen, zero in [(p, False) for p in (0, 1, 2, 3, 17)] + [(1, True)]:
                pkt = bytearray(finish_udp(_ip_packet(shape, _rand(rng, plen), rng), zero_udp=zero))
                ck = len(pkt) - plen - 2
                if not zero and pkt[ck:ck + 2] == b"\x00\x00":
                    pkt[ck:ck + 2] = b"\xff\xff"  # a computed 0 sent as 0 would be "no checksum"
                fr = self.frame(shape, pkt)
                tag = f"cut/{name}/p{plen}{'/nock' if zero else ''}"
                for flen in range(len(fr) + 1):
                    self.add(fr, flen, f"{tag}/flen={flen}")
                for t in (1, 2, 3, 17):  # Ethernet padding: not summed, nothing changes
                    self.add(fr + _rand(rng, t), len(fr) + t, f"{tag}/trailer={t}")
                if zero:
                    continue
                # the last datagram byte (or, with no payload, a port byte) off by
                # one bit: BAD_UDP with the range ending on the frame and one short
                bad = bytearray(fr)
                bad[-1 if plen else -6] ^= 0x10
                self.add(bytes(bad), len(bad), f"{tag}/badudp")
                self.add(bytes(bad) + _rand(rng, 1), len(bad) + 1, f"{tag}/badudp/trailer=1")

    # --- b. field ladder -----------------------------------------------------

    def combo(self, shape: int, base: bytes, ip_plen: int, ulen: int, tag: str) -> None:
        """`base` (an IP packet plus one trailer byte) with the IP length field
        giving ip_plen and the UDP length ulen; with the checksum the
        reference accepts and with a zero field, each without and with the
        trailer byte inside the frame."""
        v4 = shape != V6
        hl = 4 * shape if v4 else 40
        for ck in (True, False):
            ip = bytearray(base)
            if v4:
                ip[2:4] = _be16((hl + ip_plen) & 0xFFFF)
            else:
                ip[4:6] = _be16(ip_plen)
            ip[hl + 4:hl + 6] = _be16(ulen)
            if ck:
                pass_udp(ip, v4)
            else:
                ip[hl + 6:hl + 8] = b"\x00\x00"
            if v4:
                fix_ip4_cksum(ip)
            fr = self.frame(shape, ip)
            t = f"{tag}/plen={ip_plen}/ulen={ulen}/{'ck' if ck else 'nock'}"
            self.add(fr, len(fr) - 1, t)
            self.add(fr, len(fr), t + "/trailer=1")

    def field_ladder(self) -> None:
        rng = self.rng
        for shape in SHAPES:
            v4 = shape != V6
            hl = 4 * shape if v4 else 40
            name = shape_name(shape)
            for pay in (0, 4):
                base = _ip_packet(shape, _rand(rng, pay), rng) + _rand(rng, 1)
                actual = 8 + pay
                top = 65535 - hl if v4 else 65535
                tag = f"field/{name}/p{pay}"
                if shape in LADDER_BASES:
                    plens = sorted({0, 7, 8, 9, actual - 1, actual, actual + 1, top})
                    ulens = sorted({0, 7, 8, 9, actual - 1, actual, actual + 1, 65535})
                elif pay == 0:  # every other shape: both sides of ip_plen < 8 and of MIN()
                    plens, ulens = (7, 8, 9), (8,)
                else:
                    continue
                if pay == 0:
                    # A UDP frame cut around the end of its IP header is TRUNCATED
                    # on either side (room < hl + 8 follows): only a frame that
                    # ends the chain before that -- SHORT here -- tells the header
                    # check from its neighbours.
                    ip = bytearray(base)
                    if v4:
                        ip[2:4] = _be16(hl + 7)
                        fix_ip4_cksum(ip)
                    else:
                        ip[4:6] = _be16(7)
                    fr = self.frame(shape, ip)
                    for d in (-1, 0, 1):
                        self.add(fr, 14 + hl + d, f"hdrcut/{name}/room=hl{d:+d}")
                for ip_plen in plens:
                    for ulen in ulens:
                        self.combo(shape, base, ip_plen, ulen, tag)
        for shape in LADDER_BASES:
            v4 = shape != V6
            hl = 4 * shape if v4 else 40
            name = shape_name(shape)
            base = bytearray(finish_udp(_ip_packet(shape, _rand(rng, 4), rng)))
            if v4:
                # the uint16 wrap of udp.c:104: total length below, at and just past hl
                for tot in (0, hl - 1, hl, hl + 7):
                    ip = bytearray(base)
                    ip[2:4] = _be16(tot)
                    pass_udp(ip, True)
                    fix_ip4_cksum(ip)
                    self.add(self.frame(shape, ip), 14 + len(ip), f"totlen/{name}/tot={tot}")
                # only 0x20, 0x40 and 0x80 of byte 6 pass IP4_OFFMASK (ip4.h:49)
                for bit in range(16):
                    ip = bytearray(base)
                    ip[6:8] = bytes(((1 << bit) & 0xFF, (1 << bit) >> 8))
                    fix_ip4_cksum(ip)
                    self.add(self.frame(shape, ip), 14 + len(ip), f"frag/{name}/bit={bit}")
            for proto in (0, 1, 16, 17, 18, 58, 255):
                ip = bytearray(base)
                ip[9 if v4 else 6] = proto
                pass_udp(ip, v4)
                if v4:
                    fix_ip4_cksum(ip)
                self.add(self.frame(shape, ip), 14 + len(ip), f"proto/{name}/p={proto}")
            for etype in (0x0800, 0x86DD):
                for ver in range(16):
                    ip = bytearray(base)
                    ip[0] = (ver << 4) | (ip[0] & 0x0F)
                    if etype == 0x0800:
                        fix_ip4_cksum(ip)
                    self.add(self.frame(shape, ip, etype), 14 + len(ip),
                             f"version/{name}/etype={etype:04x}/v={ver}")
            for etype in (0x0800, 0x0801, 0x0008, 0x86DD, 0x86DC, 0xDD86, 0x0806, 0x8100, 0x0000,
                          0xFFFF):
                fr = self.frame(shape, base, etype)
                # (flen 13 | 14 decides nothing for an IP frame, room < 1 follows:
                # only another EtherType tells flen < 14 from its neighbours)
                for flen in (13, 14, 15, len(fr)):
                    self.add(fr, flen, f"etype/{name}/{etype:04x}/flen={flen}")

    # --- c. checksum values --------------------------------------------------

    def cksum_values(self) -> None:
        rng = self.rng
        for shape in SHAPES:
            v4 = shape != V6
            hl = 4 * shape if v4 else 40
            name = shape_name(shape)
            # a computed UDP checksum of 0: the complement in a payload word
            ip = bytearray(_ip_packet(shape, _rand(rng, 2) + bytes(2) + _rand(rng, 2), rng))
            ip[hl + 10:hl + 12] = _le16(py_oracle.payload_cksum(bytes(ip), len(ip)))
            assert py_oracle.payload_cksum(bytes(ip), len(ip)) == 0
            if v4:
                fix_ip4_cksum(ip)
            for field, what in ((b"\x00\x00", "0000"), (b"\xff\xff", "ffff"), (b"\x01\x00", "0001"),
                                (b"\xff\x7f", "7fff")):
                ip[hl + 6:hl + 8] = field
                self.add(self.frame(shape, ip), 14 + len(ip), f"ckzero/{name}/field={what}")
            if v4:  # one header bit off: BAD_IP_CKSUM before anything else is looked at
                for at in (1, 8, hl - 1):
                    bad = bytearray(ip)
                    bad[at] ^= 0x02
                    self.add(self.frame(shape, bad), 14 + len(bad), f"badip/{name}/byte={at}")
        # the most and the fewest carries in the header sum
        for fill in (0xFF, 0x00):
            for pay in (0, 5):
                ip = bytearray(ipv4_udp(_rand(rng, pay), rng, ihl=15)[0])
                ip[20:60] = bytes([fill]) * 40
                fr = self.frame(15, finish_udp(bytes(ip)))
                self.add(fr, len(fr), f"options/{fill:02x}/p{pay}")

    # --- d. IHL 0..4 ---------------------------------------------------------

    def ihl_small(self) -> None:
        """ip4_rx does not reject IHL < 5: the UDP header then lies at ip + hl
        inside the fixed header.  hl 8, 12 and 16 have the UDP length on
        address or option bytes and a header sum that can pass; hl 0 (an
        empty header sum is 0xFFFF) and hl 4 (tos and the length word cannot
        both be chosen) keep BAD_IP_CKSUM / whatever their bytes give."""
        rng = self.rng
        for ihl in range(5):
            hl = 4 * ihl
            for ip_plen in (8, 11, 12, 40):
                for ulen in (sorted({0, 8, ip_plen, 65535}) if hl >= 8 else (None,)):
                    ip = bytearray(_rand(rng, max(hl + ip_plen + 3, 24)))
                    ip[0] = 0x40 | ihl
                    ip[2:4] = _be16(hl + ip_plen)
                    ip[6:8] = b"\x40\x00"
                    ip[9] = 17
                    if ulen is not None:
                        ip[hl + 4:hl + 6] = _be16(ulen)
                        ip[hl + 6:hl + 8] = b"\xa5\x5a"
                    fix_ip4_cksum(ip)
                    u = (ip[hl + 4] << 8) | ip[hl + 5]
                    plen = hl + min(u, ip_plen)
                    rooms = sorted({19, 20, hl + 7, hl + 8, plen - 1, plen, plen + 1,
                                    hl + ip_plen - 1, hl + ip_plen, hl + ip_plen + 1})
                    tag = f"ihlsmall/ihl{ihl}/plen={ip_plen}/ulen={ulen}"
                    variants = [(bytes(ip), "asis")]
                    if hl >= 8:
                        good = self.solve(ip, hl)
                        bad = bytearray(good)
                        bad[19] ^= 0x01  # ip->dst: in every pseudo-header, in no header sum here
                        variants = [(bytes(good), "ok"), (bytes(bad), "badudp")]
                    for pkt, what in variants:
                        fr = self.frame(ihl, pkt)
                        for room in rooms:
                            if 0 <= room <= len(pkt):
                                self.add(fr, 14 + room, f"{tag}/{what}/room={room}")

    # The words tried, in turn, for the value that makes the UDP sum pass where
    # the UDP header overlaps the addresses (each outside [0, hl), so the header
    # checksum stands): udp->cksum itself, then address words.
    SOLVE_AT = {8: (14, 16, 18), 12: (18, 12, 14), 16: (22, 16, 18)}

    def solve(self, ip: bytearray, hl: int) -> bytearray:
        """All 65 536 values of one word through the C oracle in one ragged
        call; the first that gives OK.  (An overlapping word is summed twice,
        in the pseudo-header and in the range, so the complement alone does
        not do.)  Every shape of the grid has a solution: asserted."""
        fr = np.frombuffer(eth_frame(bytes(ip), np.random.default_rng(0)), np.uint8)
        n, size = 1 << 16, fr.size
        vals = np.arange(n, dtype=np.uint32)
        offs = np.arange(n, dtype=np.uint64) * np.uint64(size)
        lens = np.full(n, size, np.uint16)
        for at in self.SOLVE_AT[hl]:
            a = np.tile(fr, (n, 1))
            a[:, 14 + at] = vals & 0xFF
            a[:, 14 + at + 1] = vals >> 8
            hit = np.flatnonzero(c_oracle.rx_verdict_ragged(a.reshape(-1), offs, lens) == OK)
            if hit.size:
                out = bytearray(ip)
                out[at:at + 2] = _le16(int(hit[0]))
                return out
        raise AssertionError(f"no word makes the UDP sum of an hl {hl} frame pass")


@functools.lru_cache(maxsize=None)
def grid() -> tuple:
    g = _Grid()
    g.cut_ladder()
    g.field_ladder()
    g.cksum_values()
    g.ihl_small()
    return tuple(g.out)


# --- layouts ------------------------------------------------------------------

SLOT = 128
PAD = 64  # zero bytes after the last frame, as packets.pack leaves them


def slots(frames, seed: int = 1):
    """Scrambled 128-byte slots, each holding the whole frame_bytes: what lies
    past flen follows the frame.  -> (buf, offs uint64, lens uint16)."""
    n = len(frames)
    idx = np.random.default_rng(seed).permutation(n)
    buf = np.zeros(n * SLOT + PAD, np.uint8)
    offs = (idx * SLOT).astype(np.uint64)
    lens = np.empty(n, np.uint16)
    for i, (fr, flen, _) in enumerate(frames):
        o = int(offs[i])
        buf[o:o + len(fr)] = np.frombuffer(fr, np.uint8)
        lens[i] = flen
    return buf, offs, lens


def packed(frames, phase: int = 0):
    """Only frame[:flen] of each, back to back from byte `phase` of a 16-byte
    chunk: the next frame's Ethernet header follows immediately."""
    body = b"".join(fr[:flen] for fr, flen, _ in frames)
    lens = np.array([flen for _, flen, _ in frames], np.uint16)
    offs = np.concatenate(([0], np.cumsum(lens.astype(np.uint64))[:-1])).astype(np.uint64)
    buf = np.frombuffer(bytes(phase) + body + bytes(PAD), np.uint8).copy()
    return buf, offs + np.uint64(phase), lens


def garbled(frames, seed: int = 2):
    """The frames with both checksum fields overwritten where they lie inside
    the frame (tx_model.garble_fields): what a seal is handed."""
    import tx_model
    n = len(frames)
    buf = np.zeros(n * SLOT, np.uint8)
    offs = np.arange(n, dtype=np.uint64) * np.uint64(SLOT)
    lens = np.array([flen for _, flen, _ in frames], np.uint16)
    for i, (fr, _, _) in enumerate(frames):
        buf[i * SLOT:i * SLOT + len(fr)] = np.frombuffer(fr, np.uint8)
    tx_model.garble_fields(buf, offs, lens, np.random.default_rng(seed))
    return tuple((buf[i * SLOT:i * SLOT + len(fr)].tobytes(), flen, tag)
                 for i, (fr, flen, tag) in enumerate(frames))


def oracle_verdicts(frames) -> np.ndarray:
    buf, offs, lens = pack([(fr[:flen], flen) for fr, flen, _ in frames])
    return c_oracle.rx_verdict_ragged(buf, offs, lens)


# --- census -------------------------------------------------------------------

def frame_shape(fr: bytes) -> str:
    """The header shape from frame_bytes (the part past flen included: a cut
    frame keeps the shape it was cut from)."""
    if len(fr) < 15:
        return "none"
    etype = (fr[12] << 8) | fr[13]
    if etype == 0x0800 and fr[14] >> 4 == 4:
        return f"ihl{fr[14] & 0x0F}"
    if etype == 0x86DD and fr[14] >> 4 == 6:
        return "v6"
    return "other"


def census(frames, verdicts) -> Counter:
    """Counter over (decision, distance, shape, verdict): for each decision of
    the RX chain that a frame reaches (every earlier check passed), its
    distance from that threshold where it is -1, 0 or +1.

        "flen"      flen - 14
        "hdr"       room - max(hl, 20)  (IPv6: room - 40)
        "ip_plen"   ip_plen - 8
        "udp_hdr"   room - (hl + 8)
        "min"       ulen - ip_plen
        "ulen"      ulen - 8            (udp_len < 8: the seal, the record's wrap)
        "range"     room - (udp_len + hl), the checksum field not zero
    """
    c = Counter()

    def note(decision, dist, shape, v):
        if -1 <= dist <= 1:
            c[(decision, dist, shape, v)] += 1

    for (fr, flen, _), v in zip(frames, verdicts):
        v = int(v)
        shape = frame_shape(fr)
        note("flen", flen - 14, shape, v)
        if flen < 15 or shape in ("none", "other"):
            continue
        v4 = shape != "v6"
        room = flen - 14
        ip = fr[14:]
        hl = (ip[0] & 0x0F) * 4 if v4 else 40
        note("hdr", room - (max(hl, 20) if v4 else 40), shape, v)
        if room < (max(hl, 20) if v4 else 40):
            continue
        if v4 and (py_oracle.ip_cksum(ip[:hl]) != 0 or (ip[6] & 0x1F) or ip[7]):
            continue
        if (ip[9] if v4 else ip[6]) != 17:
            continue
        _, ip_plen = _fields(ip, v4)
        note("ip_plen", ip_plen - 8, shape, v)
        if ip_plen < 8:
            continue
        note("udp_hdr", room - (hl + 8), shape, v)
        if room < hl + 8:
            continue
        ulen = (ip[hl + 4] << 8) | ip[hl + 5]
        note("min", ulen - ip_plen, shape, v)
        note("ulen", ulen - 8, shape, v)
        if ip[hl + 6] == 0 and ip[hl + 7] == 0:
            continue
        note("range", room - (min(ulen, ip_plen) + hl), shape, v)
    return c


# --- what an off-by-one would answer ---------------------------------------------

THRESHOLDS = ("flen", "hdr", "ip_plen", "udp_hdr", "range")
WRONG_CHAINS = tuple((t, d) for t in THRESHOLDS for d in (-1, 1)) + \
    (("min", "ulen"), ("min", "ip_plen"), ("sees", 1))


def shifted_chain(frame: bytes, flen: int, which=None, by=0) -> int:
    """The RX chain of py_oracle.rx_verdict with ONE comparison moved: threshold
    `which` of THRESHOLDS raised or lowered by 1 (`<` written as `<=`, or the
    reverse); "min": MIN() replaced by one of its arguments; "sees": the chain
    reads `by` bytes past the frame, as a parse without the length mask would.
    With nothing moved it is the oracle's chain (asserted over the grid); each
    moved one is what a kernel copy with that slip would answer, so the grid
    must tell every one of them from the oracle."""
    k = {t: by if t == which else 0 for t in THRESHOLDS}
    if flen < 14 + k["flen"]:
        return TRUNCATED
    # a moved threshold reads what it let through: what lies behind the frame
    # in a slot (frame_bytes past flen, then zeros)
    f = bytes(frame) + bytes(64)
    etype = (f[12] << 8) | f[13]
    if etype not in (0x0800, 0x86DD):
        return NOT_IP
    room = flen - 14 + (by if which == "sees" else 0)
    ip = f[14:]
    if room < 1:
        return TRUNCATED
    v4 = etype == 0x0800
    if ip[0] >> 4 != (4 if v4 else 6):
        return BAD_VERSION
    hl = (ip[0] & 0x0F) * 4 if v4 else 40
    if room < (max(hl, 20) if v4 else 40) + k["hdr"]:
        return TRUNCATED
    if v4 and py_oracle.ip_cksum(ip[:hl]) != 0:
        return BAD_IP
    if v4 and ((ip[6] & 0x1F) or ip[7]):
        return FRAGMENT
    if (ip[9] if v4 else ip[6]) != 17:
        return NOT_UDP
    _, ip_plen = _fields(ip, v4)
    if ip_plen < 8 + k["ip_plen"]:
        return SHORT
    if room < hl + 8 + k["udp_hdr"]:
        return TRUNCATED
    ulen = (ip[hl + 4] << 8) | ip[hl + 5]
    udp_len = min(ulen, ip_plen) if which != "min" else ulen if by == "ulen" else ip_plen
    if ip[hl + 6] == 0 and ip[hl + 7] == 0:
        return OK_NO_CKSUM
    plen = udp_len + hl
    if room < max(plen, 20) + k["range"] or plen > len(ip):
        return TRUNCATED
    return BAD_UDP if py_oracle.payload_cksum(ip[:max(plen, 20)], plen) != 0 else OK


TX_THRESHOLDS = ("flen", "ihl", "hdr", "ip_plen", "udp_hdr", "ulen", "range")
TX_WRONG_CHAINS = tuple((t, d) for t in TX_THRESHOLDS for d in (-1, 1) if (t, d) != ("ihl", -1)) + \
    (("min", "ulen"), ("min", "ip_plen"))  # (hl < 19 is hl < 20: hl is a multiple of 4)


def shifted_seal_status(frame: bytes, flen: int, zero_udp: bool, which=None, by=0) -> int:
    """The same for the seal's chain (tx_model.seal_frame): its status with
    one comparison moved.  (The UDP header check moved down shows only with
    zero_udp: a field stored one byte past the frame; the range check only
    without.)"""
    k = {t: by if t == which else 0 for t in TX_THRESHOLDS}
    if flen < 14 + k["flen"]:
        return 7
    f = bytes(frame) + bytes(64)
    etype = (f[12] << 8) | f[13]
    if etype not in (0x0800, 0x86DD):
        return 4
    room, ip = flen - 14, f[14:]
    if room < 1:
        return 7
    v4 = etype == 0x0800
    if ip[0] >> 4 != (4 if v4 else 6):
        return 5
    hl = (ip[0] & 0x0F) * 4 if v4 else 40
    if v4 and hl < 20 + k["ihl"]:
        return 6
    if room < hl + k["hdr"]:
        return 7
    if (ip[9] if v4 else ip[6]) != 17 or (v4 and ((ip[6] & 0x1F) or ip[7])):
        return 2 if v4 else 3
    _, ip_plen = _fields(ip, v4)
    if ip_plen < 8 + k["ip_plen"]:
        return 6
    if room < hl + 8 + k["udp_hdr"]:
        return 7
    ulen = (ip[hl + 4] << 8) | ip[hl + 5]
    udp_len = min(ulen, ip_plen) if which != "min" else ulen if by == "ulen" else ip_plen
    if udp_len < 8 + k["ulen"]:
        return 6
    if zero_udp:
        return 1
    return 7 if room < hl + udp_len + k["range"] else 0


def census_table(c: Counter) -> str:
    """Frames per decision and distance, all shapes and verdicts together."""
    lines = []
    for d in ("flen", "hdr", "ip_plen", "udp_hdr", "min", "ulen", "range"):
        tot = [sum(n for (dd, k, _, _), n in c.items() if dd == d and k == dist)
               for dist in (-1, 0, 1)]
        lines.append(f"{d:8s} -1: {tot[0]:5d}   0: {tot[1]:5d}   +1: {tot[2]:5d}")
    return "\n".join(lines)
