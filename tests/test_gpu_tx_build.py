"""The TX build on the GPU (wc_tx_build_ragged / wc_tx_build_host): Ethernet,
IP and UDP headers written from a socket table, both checksums included,
against the restatement in tx_build_model.py (values from the C oracle on the
model's own frame).  Every buffer is random before the call -- header areas,
payloads, gaps -- and every comparison is of the whole buffer, gaps and guard
bytes included.
"""
import functools

import numpy as np
import pytest
import torch

import tx_build_cases as cases
import tx_build_model as model
import warpcore_amd as wc

pytestmark = pytest.mark.gpu


def dev(a: np.ndarray, d) -> torch.Tensor:
    return torch.from_numpy(np.array(a, copy=True)).to(d)  # (the shared inputs are read-only)


def table(a: np.ndarray, d):
    return dev(a.view(np.uint8), d) if a.size else None


def build(buf, offs, descs, socks, dsts, slot, d, **kw):
    """Build into a device copy of exactly buf.size bytes; everything back on
    the host: (buffer, frame lengths, status, header checksums, UDP checksums,
    error count)."""
    t = dev(buf, d)
    flen, status, hdr, udp, errors = wc.tx_build_ragged(
        t, dev(offs, d), dev(descs.view(np.uint8), d), table(socks, d), table(dsts, d), slot, **kw)
    return (t.cpu().numpy(), flen.cpu().numpy(), status.cpu().numpy(), hdr.cpu().numpy(),
            udp.cpu().numpy(), int(errors.item()))


def assert_same_bytes(got: np.ndarray, want: np.ndarray, what: str):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{what}: {bad.size} bytes differ, first at {bad[:8]}: "
                           f"got {got[bad[:8]]} want {want[bad[:8]]}")


def assert_built(got, e: model.Expect, what: str, stored: bool = True, before=None):
    buf, flen, status, hdr, udp, errors = got
    bad = np.flatnonzero(status != e.status)
    assert bad.size == 0, (f"{what}: {bad.size} status codes differ, first {bad[:8]}: "
                           f"got {status[bad[:8]]} want {e.status[bad[:8]]}")
    np.testing.assert_array_equal(flen, e.frame_len)
    np.testing.assert_array_equal(hdr, e.ip_hdr)
    np.testing.assert_array_equal(udp, e.udp)
    assert errors == e.errors
    assert_same_bytes(buf, e.buf if stored else before, what)


@functools.lru_cache(maxsize=None)
def world(layout: str, ns: int, nd: int, n: int = 600, seed: int = 0):
    """(buf, offs, descs, socks, dsts, slot) of n frames, never written."""
    rng = np.random.default_rng(1000 * seed + 7 * ns + nd + sum(layout.encode()))
    socks, dsts = cases.socks_table(rng, ns), cases.dsts_table(rng, nd)
    descs = cases.descs_for(rng, n, ns, nd)
    k = min(n, len(cases.DATA_LENS))
    descs["data_len"][:k] = cases.DATA_LENS[-k:]
    buf, offs, slot = cases.lay_out(rng, descs, socks, layout)
    for a in (buf, offs, descs, socks, dsts):
        a.setflags(write=False)
    return buf, offs, descs, socks, dsts, slot


@functools.lru_cache(maxsize=None)
def expect(layout: str, ns: int, nd: int, n: int = 600, seed: int = 0, zero_udp: bool = False):
    buf, offs, descs, socks, dsts, slot = world(layout, ns, nd, n, seed)
    return model.Expect(buf, offs, descs, socks, dsts, slot, zero_udp)


MIXES = [(name, 256, 300) for name in cases.LAYOUTS] + [
    ("slots", 1, 1), ("slots", 3, 0), ("pack_1_5", 3, 1), ("pack_1_0", 256, 0),
    ("pack_2_14", 1, 300)]


@pytest.mark.parametrize("layout,ns,nd", MIXES)
def test_build_is_byte_exact(gpu, layout, ns, nd):
    """600 frames, af 4 / 6 x connected / unconnected x ECN on / off x six TOS
    values, in scrambled 2048-B slots and packed back to back (every 16-byte
    and 4-byte phase of the header start)."""
    w = world(layout, ns, nd)
    e = expect(layout, ns, nd)
    if layout in ("pack_1_0", "pack_1_5") and ns == 256:
        assert set((w[1] % 16).tolist()) == set(range(16))
    if nd == 0 and ns > 1:  # unconnected sockets have no destination: both kinds of outcome
        assert {model.SEALED, model.MALFORMED} == set(np.unique(e.status).tolist())
    elif nd:
        assert (e.status == model.SEALED).all()
    assert not np.array_equal(e.buf, w[0])
    assert_built(build(*w, gpu), e, f"{layout} ns={ns} nd={nd}")


@pytest.mark.parametrize("shift", [0, 1])
def test_build_data_len_values(gpu, shift):
    """Every data_len of the list, IPv4 and IPv6, each at an even and an odd
    frame address."""
    rng = np.random.default_rng(40 + shift)
    socks, dsts = cases.socks_table(rng, 8), cases.dsts_table(rng, 2)
    descs = cases.descs_for(rng, 4 * len(cases.DATA_LENS), 8, 2,
                            data_lens=np.repeat(cases.DATA_LENS, 4))
    descs["sock"] = np.arange(descs.size) % 4  # v4 / v6, unconnected / connected
    buf, offs, slot = cases.lay_out(rng, descs, socks, "pack_2_0")
    buf = np.concatenate([rng.integers(0, 256, shift, dtype=np.uint8), buf])
    offs = offs + np.uint64(shift)
    assert (offs % 2 == shift).all()
    e = model.Expect(buf, offs, descs, socks, dsts, slot)
    assert (e.status == model.SEALED).all()
    assert_built(build(buf, offs, descs, socks, dsts, slot, gpu), e, f"shift={shift}")


@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_build_tile_edges(gpu, n):
    for layout in ("slots", "pack_1_5"):
        w = world(layout, 256, 300, n, seed=n)
        assert_built(build(*w, gpu), expect(layout, 256, 300, n, seed=n), f"n={n} {layout}")


def test_build_jumbo_frames(gpu):
    """The longest frames a uint16 length holds are SEALED, one byte more is
    MALFORMED; several stream rows per frame."""
    rng = np.random.default_rng(65535)
    socks, dsts = cases.socks_table(rng, 8), cases.dsts_table(rng, 1)
    descs = cases.descs_for(rng, 6, 8, 1, data_lens=(65493, 65494, 65473, 65474, 9000, 8999))
    descs["sock"] = (2, 2, 3, 3, 0, 1)  # connected IPv4 / IPv6, then unconnected ones
    slot = 65536
    buf = rng.integers(0, 256, 6 * slot + 64, dtype=np.uint8)
    offs = (np.array([3, 0, 5, 1, 2, 4], np.uint64) * np.uint64(slot)) + np.uint64(1)
    offs[0] -= np.uint64(1)
    e = model.Expect(buf, offs, descs, socks, dsts, slot - 1)
    assert e.status.tolist() == [0, 6, 0, 6, 0, 0] and e.frame_len[0] == e.frame_len[2] == 65535
    assert_built(build(buf, offs, descs, socks, dsts, slot - 1, gpu), e, "jumbo")


def test_build_every_status_in_its_order(gpu):
    """A bad sock, a table entry with af 5, a bad dst (ignored for a connected
    socket), slot_bytes one byte short, and frames that fail two checks get the
    first one's code; error frames and their whole slots are unchanged,
    frame_len is 0, and the error count accumulates across two calls."""
    rng = np.random.default_rng(66)
    socks, dsts = cases.socks_table(rng, 9), cases.dsts_table(rng, 2)
    socks["af"][8] = 5
    socks["flags"][8] = model.SOCK_CONNECTED
    slot = 142  # an IPv4 frame of 100 payload bytes fits exactly, an IPv6 one does not
    rows = [  # (sock, dst, data_len), expected status
        ((0, 1, 100), model.SEALED),
        ((9, 1, 100), model.MALFORMED),      # sock >= ns
        ((255, 0, 0), model.MALFORMED),
        ((8, 1, 100), model.MALFORMED),      # af 5
        ((0, 2, 100), model.MALFORMED),      # unconnected, dst >= ndst
        ((2, 2, 100), model.SEALED),         # connected: dst ignored
        ((2, 65535, 100), model.SEALED),
        ((0, 1, 101), model.TRUNCATED),      # one byte past slot_bytes
        ((1, 1, 81), model.TRUNCATED),       # IPv6: 62 + 81 = 143
        ((1, 1, 80), model.SEALED),
        ((0, 2, 101), model.MALFORMED),      # bad dst and too long: the first
        ((9, 2, 65535), model.MALFORMED),    # bad sock, bad dst, too long for any slot
        ((2, 0, 65494), model.MALFORMED),    # past 65535 before past the slot
        ((3, 0, 65473), model.TRUNCATED),    # 65535 bytes: fits a length, not the slot
    ] * 6  # (more than a tile: 84 frames)
    descs = cases.descs_for(rng, len(rows), 8, 2)
    for i, ((s, ds, dl), _) in enumerate(rows):
        descs["sock"][i], descs["dst"][i], descs["data_len"][i] = s, ds, dl
    buf = rng.integers(0, 256, len(rows) * 256 + 64, dtype=np.uint8)
    offs = (rng.permutation(len(rows)).astype(np.uint64) * np.uint64(256)) + np.uint64(3)
    e = model.Expect(buf, offs, descs, socks, dsts, slot)
    assert e.status.tolist() == [st for _, st in rows]
    got = build(buf, offs, descs, socks, dsts, slot, gpu)
    assert_built(got, e, "statuses")
    assert not got[1][e.status > 1].any() and e.errors == 10 * 6
    # the count accumulates
    errors = torch.full((1,), 5, dtype=torch.int64, device=gpu)
    for k in (1, 2):
        build(buf, offs, descs, socks, dsts, slot, gpu, errors=errors)
        assert int(errors.item()) == 5 + k * e.errors


@pytest.mark.parametrize("layout", ["slots", "pack_1_5"])
def test_build_zero_udp(gpu, layout):
    """WC_TX_ZERO_UDP_CKSUM: the field is written 0 and no payload byte is read
    -- the buffer ends with the headers of the last frame, whose payload is
    not there to be read, and a companion buffer with other payload bytes gives
    the same results."""
    buf, offs, descs, socks, dsts, slot = world(layout, 256, 300)
    e = expect(layout, 256, 300, zero_udp=True)
    assert (e.status == model.SEALED_ZERO_UDP).all() and not e.udp.any()
    last = int(np.argmax(offs))
    hb = int(e.frame_len[last]) - int(descs["data_len"][last])
    end = int(offs[last]) + hb  # the allocation stops where the last frame's payload would start
    got = build(buf[:end], offs, descs, socks, dsts, slot, gpu, zero_udp=True)
    want = model.Expect(buf[:end], offs, descs, socks, dsts, slot, True)
    assert_built(got, want, layout)
    other = buf[:end].copy()
    for o, fl, d in zip(offs.tolist(), e.frame_len.tolist(), descs["data_len"].tolist()):
        other[int(o) + fl - d:int(o) + fl] ^= 0xA5
    got2 = build(other, offs, descs, socks, dsts, slot, gpu, zero_udp=True)
    for a, b in zip(got[1:], got2[1:]):
        np.testing.assert_array_equal(a, b)


@pytest.mark.parametrize("layout", ["slots", "pack_1_0"])
def test_build_no_store(gpu, layout):
    w = world(layout, 256, 300)
    e = expect(layout, 256, 300)
    assert_built(build(*w, gpu, store=False), e, layout, stored=False, before=w[0])


def test_build_computed_checksum_zero(gpu):
    """A UDP checksum that comes out 0 is stored as 00 00 (udp.c:213)."""
    rng = np.random.default_rng(5)
    socks, dsts = cases.socks_table(rng, 8), cases.dsts_table(rng, 1)
    descs = cases.descs_for(rng, 4, 8, 1, data_lens=(64, 64, 65, 65))
    descs["sock"] = (2, 3, 2, 3)
    buf, offs, slot = cases.lay_out(rng, descs, socks, "pack_1_1")
    for i, (o, d) in enumerate(zip(offs.tolist(), descs)):
        at = int(o) + model.hdr_len(int(socks[int(d["sock"])]["af"])) + 10
        buf[at:at + 2] = 0  # a zero payload word at an even offset takes the complement
        c = model.Expect(buf, offs, descs, socks, dsts, slot).udp[i]
        buf[at], buf[at + 1] = c & 0xFF, c >> 8
    e = model.Expect(buf, offs, descs, socks, dsts, slot)
    assert not e.udp.any() and (e.status == model.SEALED).all()
    assert len(set((offs % 2).tolist())) == 2  # the field at an even and an odd address
    got = build(buf, offs, descs, socks, dsts, slot, gpu)
    assert_built(got, e, "zero checksum")
    for o, fl, d in zip(offs.tolist(), e.frame_len.tolist(), descs["data_len"].tolist()):
        at = int(o) + fl - d - 2
        assert got[0][at] == 0 and got[0][at + 1] == 0


@functools.lru_cache(maxsize=None)
def connected_world():
    """400 frames of 16 connected sockets in scrambled slots."""
    rng = np.random.default_rng(16)
    socks = cases.socks_table(rng, 16)
    socks["flags"] |= model.SOCK_CONNECTED
    descs = cases.descs_for(rng, 400, 16, 0)
    buf, offs, slot = cases.lay_out(rng, descs, socks, "slots")
    return buf, offs, descs, socks, cases.dsts_table(rng, 0), slot


def test_built_frames_are_delivered_and_demultiplexed(gpu):
    """Built frames through the RX side's own calls: all delivered, the records
    match the descriptors, and with a table of the peers' sockets (the tuples
    swapped) every frame finds its socket."""
    buf, offs, descs, socks, dsts, slot = connected_world()
    t = dev(buf, gpu)
    d_off = dev(offs, gpu)
    flen, status, _, _, _ = wc.tx_build_ragged(t, d_off, dev(descs.view(np.uint8), gpu),
                                               table(socks, gpu), None, slot)
    assert not status.any()
    verdicts, records, lst, cnt, drops = wc.rx_deliver_ragged(t, d_off, flen)
    n = descs.size
    sealed = t.cpu().numpy()
    zero = np.array([not sealed[int(o) + int(f) - int(d) - 2:int(o) + int(f) - int(d)].any()
                     for o, f, d in zip(offs, flen.cpu().numpy(), descs["data_len"])])
    np.testing.assert_array_equal(verdicts.cpu().numpy(),
                                  np.where(zero, wc.RX_OK_NO_CKSUM, wc.RX_OK))
    assert int(cnt.item()) == n and int(drops.item()) == 0
    np.testing.assert_array_equal(lst.cpu().numpy(), np.arange(n, dtype=np.uint32))
    rec = records.cpu().numpy().view(wc.RX_RECORD).reshape(-1)
    sk = socks[descs["sock"]]
    np.testing.assert_array_equal(rec["data_len"], descs["data_len"])
    np.testing.assert_array_equal(rec["sport"], sk["lport"])
    np.testing.assert_array_equal(rec["dport"], sk["rport"])
    np.testing.assert_array_equal(rec["af"], sk["af"])
    assert (rec["ttl"] == 255).all()
    np.testing.assert_array_equal(rec["data_off"], np.where(sk["af"] == 4, 42, 62))
    # the peers: every tuple swapped
    peers = np.zeros(socks.size, dtype=wc.RX_SOCK)
    peers["af"], peers["connected"] = socks["af"], 1
    peers["lport"], peers["rport"] = socks["rport"], socks["lport"]
    peers["laddr"], peers["raddr"] = socks["raddr"], socks["laddr"]
    tab = dev(wc.rx_socktab_build(peers), gpu)
    sock, _, _ = wc.rx_demux(t, d_off, records, tab, socks.size, want_list=False)
    np.testing.assert_array_equal(sock.cpu().numpy(), descs["sock"])


def test_seal_over_a_built_ring_changes_nothing(gpu):
    buf, offs, descs, socks, dsts, slot = connected_world()
    t = dev(buf, gpu)
    d_off = dev(offs, gpu)
    flen, status, hdr, udp, _ = wc.tx_build_ragged(t, d_off, dev(descs.view(np.uint8), gpu),
                                                   table(socks, gpu), None, slot)
    built = t.cpu().numpy()
    s2, hdr2, udp2, errors = wc.tx_seal_ragged(t, d_off, flen)
    np.testing.assert_array_equal(s2.cpu().numpy(), status.cpu().numpy())
    np.testing.assert_array_equal(hdr2.cpu().numpy(), hdr.cpu().numpy())
    np.testing.assert_array_equal(udp2.cpu().numpy(), udp.cpu().numpy())
    assert int(errors.item()) == 0
    assert_same_bytes(t.cpu().numpy(), built, "seal over a built ring")


@pytest.mark.parametrize("nt,layout", [("0", "slots"), ("1", "pack_1_5")])
def test_build_temporal_and_nontemporal_loads(gpu, monkeypatch, nt, layout):
    """Both <NT> instances, through the tuning build's WC_NT."""
    monkeypatch.setenv("WC_NT", nt)
    wc.reload_config()
    try:
        w = world(layout, 256, 300)
        assert_built(build(*w, gpu), expect(layout, 256, 300), f"WC_NT={nt}")
        assert_built(build(*w, gpu, store=False), expect(layout, 256, 300), f"WC_NT={nt} no store",
                     stored=False, before=w[0])
    finally:
        monkeypatch.delenv("WC_NT")
        wc.reload_config()


@functools.lru_cache(maxsize=None)
def host_world():
    rng = np.random.default_rng(3000)
    socks, dsts = cases.socks_table(rng, 32), cases.dsts_table(rng, 40)
    descs = cases.descs_for(rng, 3000, 32, 40)
    descs["sock"][[2, 1500]] = 200  # an error frame in the middle of either batch
    buf, offs, slot = cases.lay_out(rng, descs, socks, "slots")
    return buf, offs, descs, socks, dsts, slot


@functools.lru_cache(maxsize=None)
def host_expect(n: int, zero_udp: bool) -> model.Expect:
    ring, offs, descs, socks, dsts, slot = host_world()
    return model.Expect(ring, offs[:n], descs[:n], socks, dsts, slot, zero_udp)


@pytest.mark.parametrize("register", [False, True])
@pytest.mark.parametrize("n", [5, 3000])
@pytest.mark.parametrize("zero_udp", [False, True])
def test_build_host(gpu, register, n, zero_udp):
    """Frames in host memory, registered and pageable: the calling thread
    writes the headers, the seal's host batch computes, the calling thread
    stores; the resident server is never asked."""
    ring, offs, descs, socks, dsts, slot = host_world()
    offs, descs = offs[:n], descs[:n]
    buf = ring.copy()
    e = host_expect(n, zero_udp)
    assert e.errors == (1 if n == 5 else 2)
    if register:
        wc.host_register(buf)
    s0 = wc.server_stats()
    try:
        flen, status, errors = wc.tx_build_host(buf, offs, descs, socks, dsts, slot,
                                                zero_udp=zero_udp)
    finally:
        if register:
            wc.host_unregister(buf)
    assert wc.server_stats() == s0
    np.testing.assert_array_equal(status, e.status)
    np.testing.assert_array_equal(flen, e.frame_len)
    assert errors == e.errors
    assert_same_bytes(buf, e.buf, f"host n={n}")
