"""Records, destination tables, descriptors and peers for the TX neighbour
tests: two known-answer frames worked by hand from the reference, batches of
update records with repeats, look-alike keys and bad families, keys whose
probes wrap a small table's end, destination tables with duplicate misses, a
grid with a frame in every branch of the hold chain, and a dozen peers for the
closed loop.  The engine tables are rx_reply_cases'."""
from __future__ import annotations

import numpy as np

import rx_reply_cases as rc
import rx_reply_model as rmodel
import tx_neigh_model as model
from rx_reply_cases import A4, A6, BC4, BC6, MAC, PEER4, PEER6, PEER_MAC, SNMA6

# arp_who_has(PEER4) and icmp6_nsol(PEER6) from rc.engine_table(), by hand:
# arp.c:121-134 -- dst ff x 6, src / sha = 02:00:00:00:00:01, spa = the first
# af-4 address 10.1.0.1, tha 0, tpa 192.168.7.7.
ARP_WHO_HAS_HEX = ("ffffffffffff" "020000000001" "0806" "0001" "0800" "06" "04" "0001"
                   "020000000001" "0a010001" "000000000000" "c0a80707")
# icmp6.c:99-126 -- dst 33:33 + target bytes 12..15, IPv6 src = entry 0, dst =
# ff02::1:ff00:99, type 135, id 0x60, the target, option 01 01 + mac.  The
# checksum by hand, big-endian 16-bit words: src fe80 + 0200 + 00ff + fe00 + 0001
# = 1ff80; dst ff02 + 0001 + ff00 + 0099 -> 3fe1c; length 0020 and next header
# 003a -> 3fe76; 8700 + 6000 -> 4e576; target 2001 + 0db8 + 0099 -> 513c8; option
# 0101 + 0200 + 0001 -> 516ca; folded 16cf; complemented e930.
NSOL_HEX = ("333300000099" "020000000001" "86dd" "60000000" "0020" "3a" "ff"
            "fe80000000000000020000fffe000001" "ff0200000000000000000001ff000099"
            "8700" "e930" "60000000" "20010db8000000000000000000000099" "0101" "020000000001")

WORLDS = {"small": (11, 300, 40), "repeats": (12, 300, 9)}  # (seed, records, distinct addresses)


def mac_of(rng) -> bytes:
    return bytes((2, 0, 0, int(rng.integers(0, 256)), int(rng.integers(0, 256)),
                  int(rng.integers(0, 256))))


def addr4(i: int) -> bytes:
    return bytes((192, 168, (i >> 8) & 0xFF, i & 0xFF))


def addr6(i: int) -> bytes:
    return PEER6[:12] + i.to_bytes(4, "big")


def keys(n: int, rng=None):
    """n distinct (af, addr), both families interleaved; with rng, garbage in an
    af-4 address's bytes 4..15 (they never count)."""
    out = []
    for i in range(n):
        if i % 2:
            out.append((6, addr6(i)))
        else:
            tail = bytes(12) if rng is None else rng.integers(0, 256, 12, dtype=np.uint8).tobytes()
            out.append((4, addr4(i) + tail))
    return out


def home(af: int, addr: bytes, cap: int) -> int:
    """The entry a key's probes start at -- the table's hash restated (murmur3's
    steps over af and the four address words), used only to choose keys."""
    M = 0xFFFFFFFF
    a = (bytes(addr[:4]) + bytes(12)) if af == 4 else bytes(addr[:16])
    h = (0x9E3779B1 * af) & M
    for i in range(4):
        x = (int.from_bytes(a[4 * i:4 * i + 4], "little") * 0xCC9E2D51) & M
        x = ((x << 15) | (x >> 17)) & M
        h ^= (x * 0x1B873593) & M
        h = ((((h << 13) | (h >> 19)) & M) * 5 + 0xE6546B64) & M
    h ^= h >> 16
    h = (h * 0x85EBCA6B) & M
    h ^= h >> 13
    h = (h * 0xC2B2AE35) & M
    return (h ^ (h >> 16)) & (cap - 1)


def wrap_keys(cap: int, n: int, last: int = 8):
    """n distinct keys at home in the table's last `last` entries: with n >
    last their probes wrap the table's end."""
    out, i = [], 0
    while len(out) < n:
        for k in ((4, addr4(i) + bytes(12)), (6, addr6(i))):
            if home(*k, cap) >= cap - last and len(out) < n:
                out.append(k)
        i += 1
    return out


def lookalikes():
    """af 4 a.b.c.d and af 6 a.b.c.d:: -- different keys."""
    a = bytes((10, 9, 8, 7))
    return [(4, a + bytes(12)), (6, a + bytes(12))]


def record_world(seed: int, n: int, nkeys: int):
    """n records [(af, mac, addr)] over nkeys distinct addresses plus the two
    look-alikes: every key many times with different MACs, af 0 and af 7
    records in between."""
    rng = np.random.default_rng(seed)
    ks = keys(nkeys, rng) + lookalikes()
    out = []
    for j in range(n):
        r = int(rng.integers(0, 12))
        if r == 0:
            out.append((0, bytes(6), bytes(16)))
        elif r == 1:
            out.append((7, mac_of(rng), ks[int(rng.integers(0, len(ks)))][1]))
        else:
            af, a = ks[int(rng.integers(0, len(ks)))]
            if af == 4:  # the ignored bytes differ from record to record
                a = a[:4] + rng.integers(0, 256, 12, dtype=np.uint8).tobytes()
            out.append((af, mac_of(rng), a))
    return out, ks


def same_key_burst(n: int, seed: int = 5):
    """One key n times (inside one wave and across workgroups), a second key
    at both ends."""
    rng = np.random.default_rng(seed)
    return [(6, mac_of(rng), addr6(1))] + [(4, mac_of(rng), addr4(2) + bytes(12)) for _ in range(n)] + \
        [(6, mac_of(rng), addr6(1))]


def dst_table(entries, rng=None) -> np.ndarray:
    """[(addr bytes, port)] -> a DST array; with rng, garbage in dmac."""
    d = np.zeros(len(entries), model.DST)
    for r, (a, port) in zip(d, entries):
        a = bytes(a)
        r["addr"][:len(a)] = np.frombuffer(a, np.uint8)
        r["port"] = port
        if rng is not None:
            r["dmac"] = rng.integers(0, 256, 6, dtype=np.uint8)
    return d


def dst_world(seed: int, ndst: int, known, hit: float = 0.5):
    """(DST array, af bytes): entries drawn from `known` keys (hits) and from
    a small pool of unknown addresses (misses, so duplicates occur -- some
    adjacent, some far apart), a few with a bad family."""
    rng = np.random.default_rng(seed)
    pool = [(4, addr4(40000 + i) + bytes(12)) for i in range(max(2, ndst // 8))] + \
        [(6, addr6(50000 + i)) for i in range(max(2, ndst // 8))]
    ents, afs = [], []
    for k in range(ndst):
        if known and rng.random() < hit:
            af, a = known[int(rng.integers(0, len(known)))]
        elif k and rng.random() < 0.25 and afs[-1] in (4, 6):
            af, a = afs[-1], ents[-1][0]  # an adjacent duplicate
        else:
            af, a = pool[int(rng.integers(0, len(pool)))]
        if rng.random() < 0.04:
            af = int(rng.choice([0, 5, 7, 255]))
        if af == 4:
            a = a[:4] + rng.integers(0, 256, 12, dtype=np.uint8).tobytes()
        ents.append((a, int(rng.integers(1, 65536))))
        afs.append(af)
    return dst_table(ents, rng), np.array(afs, np.uint8)


def socks_table():
    """Sockets for the hold grid: 0 unconnected v4, 1 unconnected v6, 2 connected
    v4, 3 connected v6, 4 a bad family."""
    s = np.zeros(5, model.SOCK)
    for i, (af, fl) in enumerate(((4, 0), (6, 2), (4, 1), (6, 3), (9, 0))):
        s[i]["af"], s[i]["flags"], s[i]["lport"] = af, fl, 0x1234
        s[i]["smac"] = np.frombuffer(MAC, np.uint8)
        s[i]["dmac"] = np.frombuffer(PEER_MAC, np.uint8)
        la, ra = (A4[0], PEER4) if af == 4 else (A6[0], PEER6)
        s[i]["laddr"][:len(la)] = np.frombuffer(la, np.uint8)
        s[i]["raddr"][:len(ra)] = np.frombuffer(ra, np.uint8)
    return s


# Destinations of the hold grid: index -> (af, state)
HOLD_DSTS = [(4, model.READY), (6, model.READY), (4, model.MISS), (6, model.MISS_DUP),
             (7, model.BAD_AF), (4, model.MISS_DUP)]


def hold_grid():
    """[(name, sock, dst, code)]: a frame in every branch of the chain."""
    M = model
    return [("sock past the table", 5, 0, M.TH_MALFORMED), ("sock 255", 255, 0, M.TH_MALFORMED),
            ("bad socket family", 4, 0, M.TH_MALFORMED),
            ("connected v4, dst past the table", 2, 60000, M.TH_READY),
            ("connected v6, dst a miss", 3, 3, M.TH_READY),
            ("dst past the table", 0, 6, M.TH_MALFORMED), ("dst 65535", 1, 65535, M.TH_MALFORMED),
            ("family differs 4/6", 0, 1, M.TH_MALFORMED), ("family differs 6/4", 1, 0, M.TH_MALFORMED),
            ("bad af destination", 0, 4, M.TH_MALFORMED),
            ("ready v4", 0, 0, M.TH_READY), ("ready v6", 1, 1, M.TH_READY),
            ("held v4, miss", 0, 2, M.TH_HELD), ("held v6, dup", 1, 3, M.TH_HELD),
            ("held v4, dup", 0, 5, M.TH_HELD)]


def descs_of(pairs) -> np.ndarray:
    d = np.zeros(len(pairs), model.DESC)
    for r, (s, t) in zip(d, pairs):
        r["sock"], r["dst"], r["data_len"], r["ip_id"] = s, t, 32, 0x3412
    return d


def hold_world(n: int, seed: int = 3) -> np.ndarray:
    """n descriptors cycling through the grid's branches in a seeded order."""
    rng = np.random.default_rng(seed)
    g = hold_grid()
    idx = list(range(len(g))) * (n // len(g) + 1)
    rng.shuffle(idx)
    return descs_of([(g[i][1], g[i][2]) for i in idx[:n]])


def peers(n: int = 12):
    """n hosts on our link: [(mac, v4 address, v6 address)]."""
    return [(bytes((2, 0, 0, 0, 7, i)), bytes((10, 1, 0, 100 + i)),
             bytes.fromhex("20010db8000000000000000000000100")[:15] + bytes((0x10 + i,)))
            for i in range(n)]


def peer_engine(mac: bytes, a4: bytes, a6: bytes) -> np.ndarray:
    """One peer's own engine table."""
    snma = bytes.fromhex("ff0200000000000000000001ff") + a6[13:16]
    return rmodel.engine(mac, 1500, [(6, a6, BC6, snma), (4, a4, BC4, None)])


__all__ = ["A4", "A6", "MAC", "PEER4", "PEER6", "PEER_MAC", "SNMA6", "rc"]
