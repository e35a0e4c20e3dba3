"""Frames and layouts for the RX neighbour tests: ARP requests and replies, the
ICMPv6 neighbour solicitations and advertisements, what the chain turns away,
and the frames of other kinds that share a ring with them -- as a boundary
grid with a frame on each side of every comparison, and as seeded worlds in
scrambled 2048-byte slots or packed at every 16-byte phase.  The builders and
tables are rx_reply_cases'."""
from __future__ import annotations

import numpy as np

import rx_neigh_model as model
import rx_reply_cases as rc
import rx_reply_model as rmodel
from rx_reply_cases import A4, A6, BC4, MAC, PEER4, PEER6, PEER_MAC, SNMA6

OPT_MAC = bytes((2, 0, 0, 0, 0, 0x77))  # a link-address option that differs from the Ethernet source
ND_DST = b"\x33\x33\xff\x00\x00\x01"
BCAST = b"\xff" * 6
# (seed, frames) per layout
WORLDS = {"slots": (303, 600), "packed": (404, 600)}

# The four known answers (checked with the Python oracle and the reference's object)
NSOL_HEX = ("3333ff00000102000000000986dd6000000000203a4020010db8000000000000000000000099"
            "ff0200000000000000000001ff000001870049c100000000fe80000000000000020000fffe000001"
            "0101020000000009")
NADV_HEX = ("02000000000902000000000186dd6000000000203afffe80000000000000020000fffe000001"
            "20010db80000000000000000000000998800e64c60000000fe80000000000000020000fffe000001"
            "0201020000000001")
ARP_HEX = "ffffffffffff02000000000908060001080006040001020000000009c0a807070000000000000a010002"
IS_AT_HEX = "020000000009020000000001080600010800060400020200000000010a010002020000000009c0a80707"


def arp(op: bytes = b"\x00\x01", tpa: bytes = None, sha: bytes = PEER_MAC, spa: bytes = PEER4,
        tha: bytes = bytes(6), hrd: bytes = b"\x00\x01", pro: bytes = b"\x08\x00", hln: int = 6,
        pln: int = 4, dst: bytes = BCAST, src: bytes = PEER_MAC, pad: int = 0,
        etype: int = 0x0806) -> bytes:
    tpa = A4[0] if tpa is None else tpa
    body = hrd + pro + bytes((hln, pln)) + op + sha + spa + tha + tpa + bytes(pad)
    return rc.eth(body, etype, dst, src)


def nd(typ: int, target: bytes, opt: bytes = None, src: bytes = PEER6, dst: bytes = None,
       plen: int = None, eth_dst: bytes = ND_DST) -> bytes:
    """A solicitation (135) or advertisement (136) with a valid checksum over
    the bytes icmp6_rx sums; plen: ip6->len as sent."""
    opt = b"\x01\x01" + OPT_MAC if opt is None else opt
    dst = SNMA6[0] if dst is None else dst
    msg = bytes((typ, 0, 0, 0)) + bytes(4) + target + opt
    p = rc.ip6(msg, 58, src, dst, plen=plen)
    k = 40 + min(len(msg) if plen is None else plen, len(msg))
    ck = rc.c_oracle.payload_cksum(p[:k], k)
    return rc.eth(p[:42] + rc._le16(ck) + p[44:], 0x86DD, eth_dst, PEER_MAC)


def grid():
    """One frame on each side of every comparison of the chain and of the
    record rules: [(name, frame, action byte, engine, code)], the expectation
    stated by hand.  The action byte is what wc_rx_reply_plan wrote, or a
    stale one."""
    M, H = model, model.HOST
    E, no4 = rc.engine_table(), rc.engine_table(v4=0)
    g = []

    def add(name, fr, code, act=H, eng=E):
        g.append((name, fr, act, eng, code))

    a = arp()
    add("arp flen 42", a, M.ARP_IS_AT)
    add("arp flen 41", a[:41], M.MALFORMED)
    add("arp flen 60", arp(pad=18), M.ARP_IS_AT)
    for name, kw in (("hrd", dict(hrd=b"\x00\x02")), ("hrd low", dict(hrd=b"\x00\x00")),
                     ("hrd high byte", dict(hrd=b"\x01\x01")), ("hln 5", dict(hln=5)),
                     ("hln 7", dict(hln=7)), ("pro", dict(pro=b"\x08\x01")),
                     ("pro 07 ff", dict(pro=b"\x07\xff")), ("pln 3", dict(pln=3)),
                     ("pln 5", dict(pln=5))):
        add(f"arp {name} off by one", arp(**kw), M.NONE)
    for op, code in ((b"\x00\x00", M.NONE), (b"\x00\x01", M.ARP_IS_AT), (b"\x00\x02", M.UPDATE4),
                     (b"\x00\x03", M.NONE), (b"\x01\x00", M.NONE)):
        add(f"arp op {op.hex()}", arp(op=op), code)
    add("arp tpa second address", arp(tpa=A4[1]), M.ARP_IS_AT)
    add("arp tpa bcast", arp(tpa=BC4), M.UPDATE4)
    add("arp tpa 255.255.255.255", arp(tpa=b"\xff" * 4), M.UPDATE4)
    add("arp tpa other", arp(tpa=bytes((10, 1, 0, 3))), M.UPDATE4)
    add("arp tpa = an IPv6 entry's first bytes", arp(tpa=A6[0][:4]), M.UPDATE4)
    add("arp, no af-4 entry", a, M.NONE, eng=no4)
    add("arp reply, no af-4 entry", arp(op=b"\x00\x02"), M.NONE, eng=no4)
    add("arp short, no af-4 entry", a[:30], M.NONE, eng=no4)
    for act in (0, 2, 3, 4, 5, 8, 9, 10, 11, 12, 31, 255):
        add(f"arp, action {act}", a, M.NONE, act=act)
    add("host on an echo4 frame", rc.echo4(bytes(40)), M.NONE)
    add("host on an echo6 frame", rc.echo6(bytes(40)), M.NONE)
    add("ethertype 81 00", arp(etype=0x8100), M.NONE)
    add("ethertype 06 08", arp(etype=0x0608), M.NONE)
    add("flen 13", a[:13], M.NONE)
    add("flen 14, arp", a[:14], M.MALFORMED)

    s = nd(135, A6[0])
    assert len(s) == 86
    add("nsol flen 86", s, M.NADV)
    add("nsol flen 85", s[:85], M.NADV)
    add("nsol flen 78", s[:78], M.NADV)
    add("nsol flen 77", s[:77], M.MALFORMED)
    add("nsol flen 55", s[:55], M.MALFORMED)
    add("nsol flen 54", s[:54], M.NONE)
    add("nadv flen 78", nd(136, PEER6)[:78], M.UPDATE6)
    add("nadv flen 77", nd(136, PEER6)[:77], M.MALFORMED)
    add("nsol ip6 len 24", nd(135, A6[0], plen=24), M.NADV)
    add("nsol ip6 len 23", nd(135, A6[0], plen=23), M.NADV)
    add("nadv ip6 len 24", nd(136, PEER6, plen=24), M.UPDATE6)
    add("nadv ip6 len 23", nd(136, PEER6, plen=23), M.UPDATE6)
    for o in (b"\x01\x01", b"\x00\x01", b"\x01\x00", b"\x02\x01"):
        add(f"nsol option {o.hex()}", nd(135, A6[0], opt=o + OPT_MAC), M.NADV)
        add(f"nadv option {o.hex()}", nd(136, PEER6, opt=o + OPT_MAC), M.UPDATE6)
    add("nsol target second address", nd(135, A6[1]), M.NADV)
    add("nsol target snma", nd(135, SNMA6[0]), M.NONE)
    add("nsol target bcast", nd(135, rc.BC6), M.NONE)
    add("nsol target other", nd(135, PEER6), M.NONE)
    add("nsol target = an IPv4 entry's bytes", nd(135, A4[0] + bytes(12)), M.NONE)
    add("nsol target last byte", nd(135, A6[0][:15] + b"\x02"), M.NONE)
    add("nsol, no af-4 entry", s, M.NADV, eng=no4)
    add("nsol, action none", s, M.NONE, act=0)
    add("type 134", s[:54] + b"\x86" + s[55:], M.NONE)
    add("type 137", s[:54] + b"\x89" + s[55:], M.NONE)
    add("next header 59", s[:20] + b"\x3b" + s[21:], M.NONE)
    add("known nsol", bytes.fromhex(NSOL_HEX), M.NADV)
    add("known arp request", bytes.fromhex(ARP_HEX), M.ARP_IS_AT)
    return g


def world(seed: int, n: int):
    """n frames in a seeded mix: [(bytes, socket id or None, forced action or
    None)].  A forced action stands for a stale d_action byte: the tests
    overwrite what wc_rx_reply_plan gave that frame with it."""
    rng = np.random.default_rng(seed)
    out = []
    kinds = 22

    def mac():
        return bytes((2, 0, 0, 0, 1, int(rng.integers(0, 256))))

    def ip4a():
        return bytes((192, 168, int(rng.integers(0, 256)), int(rng.integers(1, 255))))

    def ip6a():
        return PEER6[:8] + rng.integers(0, 256, 8, dtype=np.uint8).tobytes()

    for i in range(n):
        k = int(rng.integers(0, kinds)) if i >= kinds else i
        force = None
        pad = int(rng.choice([0, 18, 5]))
        if k == 0:    # a request for us, from many hosts (sha is not always the Ethernet source)
            fr = arp(tpa=A4[int(rng.integers(0, 2))], sha=mac(), spa=ip4a(), pad=pad)
        elif k == 1:  # for another host; for the broadcast address
            tpa = bytes((10, 1, 0, int(rng.integers(3, 250)))) if rng.integers(0, 3) else BC4
            fr = arp(tpa=tpa, sha=mac(), spa=ip4a(), pad=pad)
        elif k == 2:  # a reply, unicast to us
            fr = arp(op=b"\x00\x02", sha=mac(), spa=ip4a(), tha=MAC, dst=MAC, pad=pad)
        elif k == 3:
            fr = arp(op=bytes(map(int, rng.choice([[0, 0], [0, 3], [1, 0], [0, 8]]))), pad=pad)
        elif k == 4:
            fr = arp(hrd=b"\x00\x06", pad=pad) if rng.integers(0, 2) else arp(hln=8, pad=pad)
        elif k == 5:
            fr = arp(pro=b"\x86\xdd", pad=pad) if rng.integers(0, 2) else arp(pln=16, pad=pad)
        elif k == 6:
            fr = arp(pad=pad)[:int(rng.integers(14, 42))]
        elif k == 7:
            fr = nd(135, A6[int(rng.integers(0, 2))], opt=b"\x01\x01" + mac(), src=ip6a())
        elif k == 8:  # without an option; with one of another type
            opt = b"" if rng.integers(0, 2) else b"\x0e\x01" + mac()
            fr = nd(135, A6[0], opt=opt, src=ip6a())
        elif k == 9:
            fr = nd(135, ip6a())
        elif k == 10:
            opt = bytes(map(int, rng.choice([[1, 1], [2, 1], [2, 1]]))) + mac()
            dst = A6[0] if rng.integers(0, 2) else SNMA6[0]
            fr = nd(136, ip6a(), opt=opt, src=ip6a(), dst=dst,
                    eth_dst=MAC if dst == A6[0] else ND_DST)
        elif k == 11:  # a solicitation or advertisement cut inside its target
            fr = nd(int(rng.choice([135, 136])), A6[0][:int(rng.integers(0, 16))], opt=b"")
        elif k == 12:  # ARP the MAC filter turns away
            fr = arp(dst=bytes((2, 0, 0, 0, 0, int(rng.integers(2, 9)))))
        elif k == 13:
            fr = rc.echo4(bytes(int(rng.integers(0, 64)))) if rng.integers(0, 2) else \
                rc.echo6(bytes(int(rng.integers(0, 64))))
        elif k == 14:  # a solicitation with a broken checksum
            fr = rc.flip(nd(135, A6[0]), int(rng.integers(54, 86)))
        elif k == 15:
            fr = arp(etype=int(rng.choice([0x8100, 0x0608, 0x88CC])), pad=pad)
        elif k == 16:  # stale HOST bytes on IPv6 frames that are no neighbour discovery
            fr = rc.echo6(bytes(int(rng.integers(0, 64)))) if rng.integers(0, 2) else \
                rc.eth(rc.udp_pkt(6, bytes(20), rc.PORT), 0x86DD)
            force = model.HOST
        elif k == 17:  # stale bytes on ARP frames
            fr, force = arp(pad=pad), int(rng.choice([0, 2, 3, 4, 5, 8, 9, 12]))
        elif k == 18:
            fr = rc.eth(rc.udp_pkt(4, bytes(int(rng.integers(0, 200))), rc.PORT), 0x0800)
        elif k == 19:  # a solicitation for a host that is not us, to our MAC
            fr = nd(135, A6[0][:15] + bytes((int(rng.integers(2, 255)),)), dst=A6[0], eth_dst=MAC)
        elif k == 20:  # an advertisement with a truncated option
            fr = nd(136, ip6a(), opt=b"\x01\x01" + mac())[:int(rng.integers(78, 86))]
            force = model.HOST
        else:
            fr = nd(135, A6[1], opt=b"\x01\x01" + mac(), src=ip6a(), plen=int(rng.integers(16, 24)))
        out.append((fr, 0 if k == 18 else None, force))
    return out


def actions_of(frames, eng, real=None):
    """The action bytes the neighbour plan reads: rx_reply_model's plan over
    the C oracle's verdicts (or `real`, the device's), the forced ones on top."""
    pairs = [(fr, sk) for fr, sk, _ in frames]
    if real is None:
        v = rc.verdicts_of(pairs)
        real = np.array([rmodel.plan(fr, int(v[i]), None, eng, 2048)[0]
                         for i, (fr, _) in enumerate(pairs)], np.uint8)
    act = np.array(real, np.uint8).copy()
    for i, (_, _, force) in enumerate(frames):
        if force is not None:
            act[i] = force
    return act


def layout(name, frames, seed):
    rng = np.random.default_rng(seed)
    pairs = [(f[0], f[1]) for f in frames]
    return rc.slots(pairs, rng) if name == "slots" else rc.packed(pairs, rng, seed % 16)


# What a world must hold at least 10 of, planned with engine_table(): every
# code and every NONE cause but the table's own ("no ip4": planned with
# engine_table(v4=0), where every ARP frame has it).
CENSUS = [(model.ARP_IS_AT, "request for us"), (model.UPDATE4, "request for another"),
          (model.UPDATE4, "reply"), (model.NADV, "nsol for us"), (model.UPDATE6, "nadv"),
          (model.MALFORMED, "arp short"), (model.MALFORMED, "nd short"),
          (model.NONE, "not host"), (model.NONE, "arp hw format"),
          (model.NONE, "arp proto format"), (model.NONE, "arp op"), (model.NONE, "not nd"),
          (model.NONE, "nsol for another"), (model.NONE, "other ethertype")]


def peer_requests():
    """Requests from the host of rx_reply_cases.peer_table() -- its MAC as sha
    and Ethernet source, its addresses as spa / IPv6 source -- for each of our
    addresses, so that the replies pass the peer's own filters."""
    out = [arp(tpa=t, pad=p) for t in A4 for p in (0, 18)]
    out += [nd(135, t, opt=o) for t in A6 for o in (b"\x01\x01" + PEER_MAC, b"", b"\x01\x01" + OPT_MAC)]
    return [(fr, None, None) for fr in out]
