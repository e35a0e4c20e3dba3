"""The RX demultiplex socket table on the CPU (wc_rx_socktab_*: pure host
arithmetic) against tests/rx_demux_model.py's dict, and every call of the
feature that must return before it touches a device."""
import ctypes

import numpy as np
import pytest

import rx_demux_model as model
import warpcore_amd as wc
from rx_demux_cases import be16, population
from warpcore_amd import _lib

OK, EINVAL = 0, -10001


def probes(socks, count: int, seed: int):
    """`count` lookups (af, laddr, lport, raddr, rport): a quarter exact hits
    of connected sockets, a quarter a bound socket's local pair from a random
    remote, the rest misses one field away from a socket, or random."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        if socks.size and i % 2 == 0:
            s = socks[int(rng.integers(0, socks.size))]
            (af, la, lp), remote = model.sock_tuple(s)
            alen = len(la)
            ra, rp = (remote[1], remote[2]) if remote else (rng.bytes(alen), int(rng.integers(0, 1 << 16)))
            if i % 4 == 2:  # a near miss: one byte or one port bit away from the socket
                which = int(rng.integers(0, 4))
                if which == 0:
                    k = int(rng.integers(0, alen))
                    la = la[:k] + bytes([la[k] ^ (1 << int(rng.integers(0, 8)))]) + la[k + 1:]
                elif which == 1:
                    lp ^= 1 << int(rng.integers(0, 16))
                elif which == 2:
                    k = int(rng.integers(0, alen))
                    ra = ra[:k] + bytes([ra[k] ^ (1 << int(rng.integers(0, 8)))]) + ra[k + 1:]
                else:
                    rp ^= 1 << int(rng.integers(0, 16))
            out.append((af, la, lp, ra, rp))
        else:
            af = 4 if rng.random() < 0.5 else 6
            alen = 4 if af == 4 else 16
            out.append((af, rng.bytes(alen), int(rng.integers(0, 1 << 16)), rng.bytes(alen),
                        int(rng.integers(0, 1 << 16))))
    return out


def test_model_self_checks():
    model.self_check()
    assert wc.RX_SOCK == model.SOCK
    assert (wc.RX_SOCK_NONE, wc.RX_SOCK_UNBOUND, wc.RX_DEMUX_MAX_SOCKS) == \
        (model.NONE, model.UNBOUND, model.MAX_SOCKS)


@pytest.mark.parametrize("ns", [0, 1, 2, 17, 254])
def test_build_and_lookup_against_the_model(ns):
    socks = population(ns, ns)
    table = model.Table(socks)
    tab = wc.rx_socktab_build(socks)
    assert tab.size == wc.rx_socktab_bytes(ns)
    # every socket finds itself; a connected socket's local pair from another
    # remote finds the bound socket of that pair, or nothing
    for i, s in enumerate(socks):
        (af, la, lp), remote = model.sock_tuple(s)
        ra, rp = (remote[1], remote[2]) if remote else (bytes(len(la)), 0)
        want = i if remote else table.lookup(af, la, lp, ra, rp)
        assert wc.rx_socktab_lookup(tab, af, la, lp, ra, rp) == want
        assert wc.rx_socktab_lookup(tab, af, la, lp, ra, rp ^ 0x100) == \
            table.lookup(af, la, lp, ra, rp ^ 0x100)
    ps = probes(socks, 10000, 1000 + ns)
    want = np.array([table.lookup(*p) for p in ps])
    got = np.array([wc.rx_socktab_lookup(tab, *p) for p in ps])
    assert (want == model.UNBOUND).sum() >= len(ps) // 2, "at least half the probes miss"
    if ns >= 2:
        assert (want != model.UNBOUND).sum() >= len(ps) // 8
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} lookups differ, first {[ps[i] for i in bad[:3]]}"


def test_precedence_and_lookalikes():
    """One local pair with a connected and a bound-only socket: a frame from
    the connected remote goes to the former, any other remote to the latter;
    the IPv4 and IPv6 sockets alike in four address bytes stay apart."""
    socks = population(17, 5)
    tab = wc.rx_socktab_build(socks)
    a4, a6 = bytes([10, 1, 0, 1]), bytes([10, 1, 0, 1]) + bytes([1] * 12)
    peer4, peer6 = bytes([192, 168, 7, 7]), bytes(range(32, 48))
    assert wc.rx_socktab_lookup(tab, 4, a4, be16(4433), peer4, be16(999)) == 1
    assert wc.rx_socktab_lookup(tab, 4, a4, be16(4433), peer4, be16(1000)) == 4
    assert wc.rx_socktab_lookup(tab, 4, a4, be16(4433), peer4, be16(998)) == 0
    assert wc.rx_socktab_lookup(tab, 4, a4, be16(4433), bytes([192, 168, 7, 8]), be16(999)) == 0
    assert wc.rx_socktab_lookup(tab, 6, a6, be16(4433), peer6, be16(999)) == 3
    assert wc.rx_socktab_lookup(tab, 6, a6, be16(4433), peer4 + peer6[4:], be16(999)) == 2
    assert wc.rx_socktab_lookup(tab, 6, a4 + bytes(12), be16(4433), peer6, be16(999)) == \
        wc.RX_SOCK_UNBOUND
    assert wc.rx_socktab_lookup(tab, 5, a6, be16(4433), peer6, be16(999)) == wc.RX_SOCK_UNBOUND


def test_ignored_bytes_do_not_matter():
    """pad, IPv4 address bytes 4..15 and a bound socket's remote: two lists
    that differ only there give the same table bytes."""
    clean = population(254, 9)
    noisy = clean.copy()
    rng = np.random.default_rng(10)
    noisy["pad"] = rng.integers(0, 1 << 16, noisy.size)
    v4, bound = noisy["af"] == 4, noisy["connected"] == 0
    noisy["laddr"][v4, 4:] = rng.integers(0, 256, (int(v4.sum()), 12))
    noisy["raddr"][v4, 4:] = rng.integers(0, 256, (int(v4.sum()), 12))
    noisy["raddr"][bound] = rng.integers(0, 256, (int(bound.sum()), 16))
    noisy["rport"][bound] = rng.integers(0, 1 << 16, int(bound.sum()))
    assert (noisy.tobytes() != clean.tobytes())
    assert wc.rx_socktab_build(noisy).tobytes() == wc.rx_socktab_build(clean).tobytes()


def test_build_behaviour():
    lib = _lib.load()
    socks = population(254, 3)
    assert wc.rx_socktab_build(socks).tobytes() == wc.rx_socktab_build(socks.copy()).tobytes()
    sizes = [wc.rx_socktab_bytes(ns) for ns in range(0, 300)]
    assert sizes[0] > 0 and all(b >= a for a, b in zip(sizes, sizes[1:]))
    tab = np.zeros(sizes[254] // 4, np.uint32)

    def build(s, ns=None):
        s = np.ascontiguousarray(s, dtype=model.SOCK).reshape(-1)
        return lib.wc_rx_socktab_build(s.ctypes.data, s.size if ns is None else ns,
                                       tab.ctypes.data)
    assert build(socks) == OK and build(socks[:0]) == OK
    assert lib.wc_rx_socktab_build(None, 0, tab.ctypes.data) == OK  # ns = 0 is valid
    # too many, NULL pointers
    assert build(socks, 255) == EINVAL
    assert lib.wc_rx_socktab_build(socks.ctypes.data, 4, None) == EINVAL
    assert lib.wc_rx_socktab_build(None, 4, tab.ctypes.data) == EINVAL
    # every bad field
    for field, values in (("af", (0, 1, 2, 3, 5, 7, 10, 255)), ("connected", (2, 3, 255))):
        for v in values:
            for at in (0, 7, 16):
                s = socks[:17].copy()
                s[field][at] = v
                assert build(s) == EINVAL, (field, v, at)
                assert not model.valid(s)
    # every kind of duplicate, once the ignored bytes are dropped
    for i in range(17):
        s = np.concatenate([socks[:17], socks[i:i + 1]])
        dup = s[-1:]
        dup["pad"] ^= 0x5A5A
        if dup["af"][0] == 4:
            dup["laddr"][0, 4:] ^= 0xFF
            dup["raddr"][0, 4:] ^= 0xFF
        if not dup["connected"][0]:
            dup["raddr"][0] ^= 0x3C
            dup["rport"] ^= 0x1111
        assert not model.valid(s) and build(s) == EINVAL, i
        assert build(np.roll(s, 1)) == EINVAL
    # ... and the mirror raises
    with pytest.raises(ValueError):
        wc.rx_socktab_build(np.concatenate([socks[:3], socks[:1]]))
    with pytest.raises(ValueError):
        wc.rx_socktab_build(np.zeros(255, model.SOCK))


def test_demux_scratch_is_arithmetic():
    lib = _lib.load()
    assert lib.wc_rx_demux_scratch(0) == 0
    prev = 0
    for n in range(0, 70001):
        b = lib.wc_rx_demux_scratch(n)
        assert b >= prev and (n == 0 or b >= 4 * 255)
        prev = b
    assert lib.wc_rx_demux_scratch(1 << 32) >= prev


def test_demux_argument_errors_need_no_gpu():
    """wc_rx_demux and wc_rx_demux_host reject bad arguments before they touch
    a device: none of these calls reaches HIP."""
    lib = _lib.load()
    p = 0x100000  # never dereferenced: every call below returns first
    # a list without its starts (or the reverse) comes first, for n = 0 too
    assert lib.wc_rx_demux(p, p, p, 8, p, 1, p, p, None, p, None) == EINVAL
    assert lib.wc_rx_demux(p, p, p, 8, p, 1, p, None, p, p, None) == EINVAL
    assert lib.wc_rx_demux(None, None, None, 0, None, 0, None, p, None, None, None) == EINVAL
    assert lib.wc_rx_demux(None, None, None, 0, None, 0, None, None, p, None, None) == EINVAL
    # n = 0 without a list looks at nothing
    assert lib.wc_rx_demux(None, None, None, 0, None, 0, None, None, None, None, None) == OK
    # too many frames, too many sockets (n = 0 included)
    assert lib.wc_rx_demux(p, p, p, (1 << 32) + 1, p, 1, p, None, None, None, None) == EINVAL
    assert lib.wc_rx_demux(p, p, p, 8, p, 255, p, None, None, None, None) == EINVAL
    assert lib.wc_rx_demux(None, None, None, 0, None, 255, None, None, None, None, None) == EINVAL
    # NULL pointers
    for k in (0, 1, 2, 4, 6):
        a = [p, p, p, 8, p, 1, p, None, None, None, None]
        a[k] = None
        assert lib.wc_rx_demux(*a) == EINVAL, k
    # records not 16-byte, table not 4-byte aligned
    assert lib.wc_rx_demux(p, p, p + 8, 8, p, 1, p, None, None, None, None) == EINVAL
    assert lib.wc_rx_demux(p, p, p, 8, p + 2, 1, p, None, None, None, None) == EINVAL
    # a list without a scratch, or with one not 4-byte aligned
    assert lib.wc_rx_demux(p, p, p, 8, p, 1, p, p, p, None, None) == EINVAL
    assert lib.wc_rx_demux(p, p, p, 8, p, 1, p, p, p, p + 2, None) == EINVAL

    buf = np.zeros(4096, np.uint8)
    off, ln = np.array([100], np.uint64), np.array([60], np.uint16)
    v, sk = np.zeros(1, np.uint8), np.zeros(1, np.uint8)
    rec = np.zeros(1, wc.RX_RECORD)
    lst, start = np.zeros(1, np.uint32), np.full(256, 7, np.uint64)
    tab = wc.rx_socktab_build(population(2, 1))
    b, o, l_, t, vv, r, s, li, st = (a.ctypes.data for a in (buf, off, ln, tab, v, rec, sk, lst,
                                                             start))

    def host(**kw):
        a = dict(b=b, nb=buf.size, o=o, l=l_, n=1, t=t, ns=2, v=vv, r=r, s=s, li=li, st=st, d=None)
        a.update(kw)
        return lib.wc_rx_demux_host(*a.values())
    assert host(st=None) == EINVAL and host(li=None) == EINVAL
    assert host(n=0, li=None) == EINVAL
    drops = ctypes.c_uint64(7)
    assert host(n=0, d=ctypes.byref(drops)) == OK and drops.value == 0 and not start.any()
    assert host(n=(1 << 32) + 1) == EINVAL and host(ns=255) == EINVAL
    for k in ("b", "o", "l", "t", "v", "r", "s"):
        assert host(**{k: None}) == EINVAL, k
    assert host(ns=3) == EINVAL          # a table built for another count
    assert host(t=b) == EINVAL           # not a table at all
    off[0] = 4090                        # the frame runs past the region
    assert host() == EINVAL
