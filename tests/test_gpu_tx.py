"""The TX seal on the GPU (wc_tx_seal_ragged / wc_tx_seal_host): both
checksums computed with their fields taken as 0 and stored raw into the
frames, against the restatement in tx_model.py (check chain in the header's
order, values from the C oracle on a copy of the frame with the fields
zeroed).  Frames are the RX ring's cases (packets.py), both checksum fields
then overwritten with 0x00 / 0xFF / random bytes; every comparison is of the
whole buffer, gaps and guard bytes included.
"""
import functools

import numpy as np
import pytest
import torch

import tx_model
import warpcore_amd as wc
from oracle import c_oracle
from packets import (RX_CASES, eth_frame, finish_udp, ipv4_udp, ipv6_udp, pack, rx_frame, rx_ring,
                     slot_ring)

pytestmark = pytest.mark.gpu

ALL_STATUS = set(range(8))
# ok4opt first: every prefix of a ring built from these holds IPv4 options
CASES_OPT_FIRST = ("ok4opt",) + tuple(c for c in RX_CASES if c != "ok4opt")


def dev(a: np.ndarray, d) -> torch.Tensor:
    return torch.from_numpy(np.array(a, copy=True)).to(d)  # (the shared layouts are read-only)


LAYOUTS = ("slots", "pack_1_0", "pack_1_5", "pack_2_14", "pack_16_3")


@functools.lru_cache(maxsize=None)
def frames_600():
    return rx_ring(np.random.default_rng(2024), 30 * len(RX_CASES), max_payload=1472)


@functools.lru_cache(maxsize=None)
def layout(name: str):
    """(buf, offs, lens) of the 600 frames in one layout, fields garbled; shared
    by the tests and never written."""
    rng = np.random.default_rng(len(name) * 131 + sum(name.encode()))
    frames = frames_600()
    if name == "slots":
        buf, offs, lens = slot_ring(frames, rng=rng)
    else:
        _, align, lead = name.split("_")
        buf, offs, lens = pack(frames, align=int(align), lead=int(lead))
    tx_model.garble_fields(buf, offs, lens, rng)
    for a in (buf, offs, lens):
        a.setflags(write=False)
    return buf, offs, lens


@functools.lru_cache(maxsize=None)
def expect(name: str, zero_udp: bool = False) -> tx_model.Expect:
    return tx_model.Expect(*layout(name), zero_udp=zero_udp)


def seal(buf, offs, lens, d, **kw):
    """Seal a device copy of exactly buf.size bytes; everything back on the host."""
    t = dev(buf, d)
    status, hdr, udp, errors = wc.tx_seal_ragged(t, dev(offs, d), dev(lens, d), **kw)
    return (t.cpu().numpy(), status.cpu().numpy(), hdr.cpu().numpy(), udp.cpu().numpy(),
            int(errors.item()))


def assert_same_bytes(got: np.ndarray, want: np.ndarray, what: str):
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{what}: {bad.size} bytes differ, first at {bad[:8]}: "
                           f"got {got[bad[:8]]} want {want[bad[:8]]}")


def assert_sealed(got, e: tx_model.Expect, what: str):
    buf, status, hdr, udp, errors = got
    bad = np.flatnonzero(status != e.status)
    assert bad.size == 0, (f"{what}: {bad.size} status codes differ, first {bad[:8]}: "
                           f"got {status[bad[:8]]} want {e.status[bad[:8]]}")
    np.testing.assert_array_equal(hdr, e.ip_hdr)
    np.testing.assert_array_equal(udp, e.udp)
    assert errors == e.errors
    assert_same_bytes(buf, e.buf, what)


@pytest.mark.parametrize("name", LAYOUTS)
def test_seal_is_byte_exact(gpu, name):
    """The whole buffer after the call equals the expected one, for frames in
    scrambled 2048-B slots and packed back to back at odd alignments (odd
    field addresses, frames sharing 16-B chunks)."""
    buf, offs, lens = layout(name)
    e = expect(name)
    assert set(np.unique(e.status).tolist()) == ALL_STATUS - {wc.TX_SEALED_ZERO_UDP}
    assert not np.array_equal(e.buf, buf)
    assert_sealed(seal(buf, offs, lens, gpu), e, name)


def rx_allowed(e: tx_model.Expect, sealed: np.ndarray, offs) -> list:
    """Per frame, the RX verdicts a sealed frame of that TX status may get."""
    out = []
    for s, o in zip(e.seals, offs.tolist()):
        if s.status == wc.TX_SEALED:
            at = int(o) + 14 + s.hl + 6
            zero = sealed[at] == 0 and sealed[at + 1] == 0
            out.append({wc.RX_OK_NO_CKSUM} if zero else {wc.RX_OK})
        else:
            out.append({wc.TX_SEALED_ZERO_UDP: {wc.RX_OK_NO_CKSUM},
                        wc.TX_IP_ONLY: {wc.RX_NOT_UDP, wc.RX_FRAGMENT},
                        wc.TX_NOT_UDP: {wc.RX_NOT_UDP},
                        wc.TX_NOT_IP: {wc.RX_NOT_IP},
                        wc.TX_BAD_VERSION: {wc.RX_BAD_VERSION}}.get(s.status))
    return out


def assert_round_trip(sealed: np.ndarray, offs, lens, e, d):
    t = dev(sealed, d)
    got_gpu, _ = wc.rx_verdict_ragged(t, dev(offs, d), dev(lens, d))
    got_gpu = got_gpu.cpu().numpy()
    got_cpu = c_oracle.rx_verdict_ragged(sealed, offs, lens)
    for i, allowed in enumerate(rx_allowed(e, sealed, offs)):
        if allowed is None:  # MALFORMED / TRUNCATED: untouched, no RX promise
            continue
        assert int(got_gpu[i]) in allowed and int(got_cpu[i]) in allowed, (
            f"frame {i}: TX status {e.seals[i].status}, RX verdict gpu {got_gpu[i]} "
            f"oracle {got_cpu[i]}, allowed {sorted(allowed)}")


@pytest.mark.parametrize("name", ("slots", "pack_1_5"))
def test_sealed_frames_pass_the_rx_checks(gpu, name):
    """A sealed frame is one wc_rx_verdict_* accepts (and the oracle's RX
    restatement too)."""
    buf, offs, lens = layout(name)
    sealed = seal(buf, offs, lens, gpu)[0]
    assert_round_trip(sealed, offs, lens, expect(name), gpu)


@pytest.mark.parametrize("name", ("slots", "pack_1_0"))
def test_seal_is_idempotent(gpu, name):
    buf, offs, lens = layout(name)
    first = seal(buf, offs, lens, gpu)
    again = seal(first[0], offs, lens, gpu)
    assert_same_bytes(again[0], first[0], name)
    np.testing.assert_array_equal(again[1], first[1])
    assert_sealed(again, expect(name), name)


@pytest.mark.parametrize("name", LAYOUTS)
def test_seal_zero_udp(gpu, name):
    """WC_TX_ZERO_UDP_CKSUM: the header checksum and udp->cksum = 0; a companion
    buffer whose payload bytes differ gives the same results (none is read)."""
    buf, offs, lens = layout(name)
    e = expect(name, True)
    assert wc.TX_SEALED_ZERO_UDP in e.status and wc.TX_SEALED not in e.status
    assert (set(np.unique(e.status).tolist()) | set(np.unique(expect(name).status).tolist())
            == ALL_STATUS)
    got = seal(buf, offs, lens, gpu, zero_udp=True)
    assert_sealed(got, e, name)
    other, want = buf.copy(), e.buf.copy()
    for s, o, flen in zip(e.seals, offs.tolist(), lens.tolist()):
        if s.status == wc.TX_SEALED_ZERO_UDP:
            lo, hi = int(o) + 14 + s.hl + 8, int(o) + flen
            other[lo:hi] ^= 0xA5
            want[lo:hi] ^= 0xA5
    got2 = seal(other, offs, lens, gpu, zero_udp=True)
    assert_same_bytes(got2[0], want, name + " (payload altered)")
    for a, b in zip(got[1:], got2[1:]):
        np.testing.assert_array_equal(a, b)
    if name == "slots":
        assert_round_trip(got[0], offs, lens, e, gpu)


@pytest.mark.parametrize("name", ("slots", "pack_1_5"))
def test_seal_no_store(gpu, name):
    """store=False: the buffer is unchanged, the value arrays hold what the
    storing call stores, 0 where nothing is computed."""
    buf, offs, lens = layout(name)
    e = expect(name)
    got = seal(buf, offs, lens, gpu, store=False)
    assert_same_bytes(got[0], buf, name)
    np.testing.assert_array_equal(got[1], e.status)
    np.testing.assert_array_equal(got[2], e.ip_hdr)
    np.testing.assert_array_equal(got[3], e.udp)
    assert got[4] == e.errors
    nothing = ~np.isin(e.status, (wc.TX_SEALED, wc.TX_SEALED_ZERO_UDP, wc.TX_IP_ONLY))
    assert not got[2][nothing].any() and not got[3][nothing].any()
    assert not got[3][e.status != wc.TX_SEALED].any()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 209])
def test_seal_tile_edges(gpu, n):
    """One frame, a tile less one, a tile, a tile plus one, three tiles and a
    partial one; IPv4 options (IHL 6..15) in every run."""
    rng = np.random.default_rng(100 + n)
    frames = rx_ring(rng, n, cases=CASES_OPT_FIRST)
    for packed in (False, True):
        buf, offs, lens = pack(frames, 1, 3) if packed else slot_ring(frames, rng=rng)
        tx_model.garble_fields(buf, offs, lens, rng)
        e = tx_model.Expect(buf, offs, lens)
        assert e.seals[0].hl > 20 and e.status[0] == wc.TX_SEALED
        assert_sealed(seal(buf, offs, lens, gpu), e, f"n={n} packed={packed}")


SEAM_IHL = (5, 9, 10, 11, 15)  # hl 40 is the last one-round header, 44 the first two-round one


@functools.lru_cache(maxsize=None)
def seam_frames():
    """Valid IPv4 UDP frames at each IHL of SEAM_IHL and IPv6 ones, payloads of
    1 and 18 bytes (the UDP fields in the frame's chunk 2, 3 or 4, the checked
    range odd and even), two of each; then one ihl_small frame.  Returns the
    frames and the header length of each but the last."""
    rng = np.random.default_rng(4044)
    frames, hls = [], []
    for _ in range(2):
        for plen in (1, 18):
            payload = rng.integers(0, 256, plen, dtype=np.uint8).tobytes()
            for ihl in SEAM_IHL:
                fr = eth_frame(finish_udp(ipv4_udp(payload, rng, ihl=ihl)[0]), rng)
                frames.append((fr, len(fr)))
                hls.append(4 * ihl)
            fr = eth_frame(finish_udp(ipv6_udp(payload, rng)[0]), rng, 0x86DD)
            frames.append((fr, len(fr)))
            hls.append(40)
    frames.append(rx_frame(rng, "ihl_small", max_payload=18))
    return frames, hls


@pytest.mark.parametrize("phase", range(16))
def test_parse_seam_every_phase(gpu, phase):
    """The boundary between the one-round and the two-round header parse
    (IHL 10 | 11) with every frame of the buffer starting at byte `phase` of a
    16-byte chunk: the RX verdicts equal the oracle's, and the seal of the
    same frames with their fields garbled is byte-exact."""
    frames, hls = seam_frames()
    buf, offs, lens = pack(frames, align=16)  # (pack aligns after its lead: shift the buffer)
    buf, offs = np.concatenate([np.zeros(phase, np.uint8), buf]), offs + np.uint64(phase)
    assert (offs % 16 == phase).all() and len(frames) < 64
    want = c_oracle.rx_verdict_ragged(buf, offs, lens)
    assert np.isin(want[:-1], (wc.RX_OK, wc.RX_OK_NO_CKSUM)).all() and wc.RX_OK in want
    got, drops = wc.rx_verdict_ragged(dev(buf, gpu), dev(offs, gpu), dev(lens, gpu))
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    assert int(drops.item()) == int(np.isin(want, wc.RX_DROPS).sum())

    tx_model.garble_fields(buf, offs, lens, np.random.default_rng(phase))
    e = tx_model.Expect(buf, offs, lens)
    assert (e.status[:-1] == wc.TX_SEALED).all() and e.status[-1] == wc.TX_MALFORMED
    assert [s.hl for s in e.seals[:-1]] == hls
    assert_sealed(seal(buf, offs, lens, gpu), e, f"phase={phase}")


def test_seal_jumbo_frames(gpu):
    """Frames of up to 9000 B: several stream rows per frame."""
    rng = np.random.default_rng(8958)
    frames = rx_ring(rng, 3 * len(RX_CASES), cases=CASES_OPT_FIRST, max_payload=8958)
    buf, offs, lens = slot_ring(frames, slot=9216, rng=rng)
    tx_model.garble_fields(buf, offs, lens, rng)
    e = tx_model.Expect(buf, offs, lens)
    assert int(lens.max()) > 6000 and (e.status == wc.TX_SEALED).sum() >= 12
    got = seal(buf, offs, lens, gpu)
    assert_sealed(got, e, "jumbo")
    assert_round_trip(got[0], offs, lens, e, gpu)


def test_seal_frames_at_buffer_end(gpu):
    """Each frame in a tensor of exactly its length: the length bounds every
    load and store."""
    rng = np.random.default_rng(9)
    frames = rx_ring(rng, 3 * len(RX_CASES))
    zero_off = np.zeros(1, np.uint64)
    seen = set()
    for fr, flen in frames:
        buf = np.frombuffer(fr[:flen], np.uint8).copy()
        lens = np.array([flen], np.uint16)
        tx_model.garble_fields(buf, zero_off, lens, rng)
        e = tx_model.Expect(buf, zero_off, lens)
        seen.add(int(e.status[0]))
        if buf.size == 0:
            buf = e.buf = np.zeros(1, np.uint8)
        assert_sealed(seal(buf, zero_off, lens, gpu), e, f"flen={flen}")
    assert len(seen) >= 6


def test_seal_computed_checksum_zero(gpu):
    """A UDP checksum that comes out 0 is stored as 0 (udp.c:213): status
    SEALED, field bytes 00 00, and the receiver takes it as "no checksum"."""
    rng = np.random.default_rng(5)
    pkt, ln = ipv4_udp(bytes(64), rng)
    ip = bytearray(pkt)
    c = c_oracle.payload_cksum(bytes(ip), ln)  # (both fields are 0 as built)
    ip[28 + 10:28 + 12] = bytes((c & 0xFF, c >> 8))  # a zero payload word, even offset from ip
    assert c_oracle.payload_cksum(bytes(ip), ln) == 0
    ip[10:12] = b"\xff\xff"
    ip[26:28] = b"\xff\xff"
    fr = eth_frame(bytes(ip), rng)
    for lead in (0, 1):  # field at an even and at an odd address
        buf, offs, lens = pack([(fr, len(fr))], 1, lead)
        e = tx_model.Expect(buf, offs, lens)
        got = seal(buf, offs, lens, gpu)
        assert_sealed(got, e, f"lead={lead}")
        at = int(offs[0]) + 14 + 20 + 6
        assert got[1][0] == wc.TX_SEALED and got[3][0] == 0
        assert got[0][at] == 0 and got[0][at + 1] == 0
        rx, _ = wc.rx_verdict_ragged(dev(got[0], gpu), dev(offs, gpu), dev(lens, gpu))
        assert int(rx.item()) == wc.RX_OK_NO_CKSUM
        assert c_oracle.rx_verdict_ragged(got[0], offs, lens)[0] == wc.RX_OK_NO_CKSUM


@functools.lru_cache(maxsize=None)
def host_ring():
    rng = np.random.default_rng(6000)
    frames = rx_ring(rng, 6000, max_payload=1472)
    buf, offs, lens = slot_ring(frames, rng=rng)
    tx_model.garble_fields(buf, offs, lens, rng)
    return buf, offs, lens


@functools.lru_cache(maxsize=None)
def host_expect(n: int, zero_udp: bool) -> tx_model.Expect:
    buf, offs, lens = host_ring()
    return tx_model.Expect(buf, offs[:n], lens[:n], zero_udp=zero_udp)


@pytest.mark.parametrize("register", [False, True])
@pytest.mark.parametrize("n", [64, 4096, 6000])
@pytest.mark.parametrize("zero_udp", [False, True])
def test_seal_host(gpu, register, n, zero_udp):
    """Frames in host memory: a zero-copy launch, in-place streaming or the
    pipeline compute, the calling thread stores; the resident server is never
    asked."""
    ring, offs, lens = host_ring()
    offs, lens = offs[:n], lens[:n]
    buf = ring.copy()
    e = host_expect(n, zero_udp)
    if register:
        wc.host_register(buf)
    s0 = wc.server_stats()
    try:
        status, errors = wc.tx_seal_host(buf, offs, lens, zero_udp=zero_udp)
    finally:
        if register:
            wc.host_unregister(buf)
    assert wc.server_stats() == s0
    np.testing.assert_array_equal(status, e.status)
    assert errors == e.errors
    assert_same_bytes(buf, e.buf, f"host n={n}")


def test_seal_host_large_registered(gpu):
    """65536 + 512 frames of a registered region: more than one launch of the
    in-place stream, the hand-over between its chunks crossed.  The ring is a
    512-frame pool tiled into slots; the expected values come from the C
    oracle's batch calls on a copy with the fields zeroed."""
    rng = np.random.default_rng(512)
    pool = rx_ring(rng, 512, max_payload=1472)
    pbuf, poffs, plens = slot_ring(pool, pad=0)
    tx_model.garble_fields(pbuf, poffs, plens, rng)
    pe = tx_model.Expect(pbuf, poffs, plens)
    reps = 129
    n = reps * 512
    assert n == 65536 + 512
    buf = np.tile(pbuf.reshape(512, 2048), (reps, 1)).reshape(-1).copy()
    offs = np.arange(n, dtype=np.int64) * 2048
    lens = np.tile(plens, reps)
    status = np.tile(pe.status, reps)
    hl = np.tile(np.array([s.hl for s in pe.seals], np.int64), reps)
    ulen = np.tile(np.array([s.udp_len for s in pe.seals], np.int64), reps)
    v4 = np.tile(np.array([len(s.stores) and s.stores[0][0] == 24 for s in pe.seals], bool), reps)
    want = buf.copy()
    ipst = np.flatnonzero(v4 & np.isin(status, (wc.TX_SEALED, wc.TX_IP_ONLY)))
    udpst = np.flatnonzero(status == wc.TX_SEALED)
    ip_at = offs[ipst] + 24
    udp_at = offs[udpst] + 14 + hl[udpst] + 6
    for at in (ip_at, udp_at):
        want[at] = 0
        want[at + 1] = 0
    ipv = c_oracle.cksum_ragged(want, offs[ipst] + 14, hl[ipst].astype(np.uint16), kind=0)
    udpv = c_oracle.cksum_ragged(want, offs[udpst] + 14,
                                 (hl[udpst] + ulen[udpst]).astype(np.uint16), kind=1)
    for at, v in ((ip_at, ipv), (udp_at, udpv)):
        want[at] = v & 0xFF
        want[at + 1] = v >> 8
    assert_same_bytes(want[:pbuf.size], pe.buf, "the batch expectation and the per-frame one")
    wc.host_register(buf)
    s0 = wc.server_stats()
    try:
        got, errors = wc.tx_seal_host(buf, offs, lens)
    finally:
        wc.host_unregister(buf)
    assert wc.server_stats() == s0
    np.testing.assert_array_equal(got, status)
    assert errors == int(np.isin(status, wc.TX_ERRORS).sum())
    assert_same_bytes(buf, want, "host n=65536+512")


def test_c_tx_seal_loop(gpu, tmp_path):
    """INTEGRATION.md section 3's seal hook compiled in C and driven like w_tx
    (tests/c/tx_seal_loop.c): headers built with garbage in both checksum
    fields, ONE wc_tx_seal_host call per queue and no store pass; every frame
    byte-identical to the oracle's and accepted by the RX checks."""
    import subprocess

    from cprog import build
    exe = build("tx_seal_loop", tmp_path)
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "tx_seal_loop: ok" in r.stdout
