"""The restatements against the code they restate (no GPU): oracle/wc_oracle.c
and oracle/py_oracle.py compared with the reference's own in_cksum.c, compiled
unchanged into oracle/_ref/libwc_ref.so (oracle/ref_oracle.py).

Every other test of this project ends in "bit-exact against the oracle"; this
module is where the oracle itself is held to the reference, over the inputs
where in_cksum.c differs from a textbook checksum: any version nibble but 4
takes the IPv6 branch, the IPv4 pseudo-header length is truncated to 16 bits,
next_hdr << 24 wraps a uint32, len - hl is converted to uint32, the result is
a native word.  The C comparison is exhaustive; py_oracle, which loops over
bytes, is compared on a subsample of a few hundred cases of each set.

The only inputs left out are payload_cksum calls with len < header length:
the reference reads ~4 GiB there, so nothing may hand it such a call
(test_guard_refuses_len_below_header_length).

A test skips only where there is neither the object nor a reference tree to
build it from; the kernels are then still held to the results recorded from
it (tests/golden/ref_vectors.npz, tests/test_gpu_parity.py).
"""
import numpy as np
import pytest

import refcases
import tx_model
from oracle import c_oracle, py_oracle, ref_oracle
from packets import pack, random_packets, rx_ring

PY_SAMPLE = 300


@pytest.fixture(scope="module")
def ref():
    if not ref_oracle.available():
        pytest.skip("no oracle/_ref/libwc_ref.so and no reference tree (WC_REFERENCE_DIR) to "
                    "build it from: the live comparison with the reference cannot run here")
    return ref_oracle


def assert_payload_domain(buf, offs, lens, count):
    """All `count` generated cases are compared: none has len < hl."""
    assert offs.size == lens.size == count
    assert (lens.astype(np.int64) >= refcases.hdr_len(buf[offs.astype(np.int64)])).all()


def assert_c_matches(ref, buf, offs, lens, kind, what):
    want = ref.cksum_ragged(buf, offs, lens, kind=kind)
    got = c_oracle.cksum_ragged(buf, offs, lens, kind=kind)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, (f"{what}: {bad.size} of {want.size} differ from the reference, first "
                           f"index {bad[:5]}, len {lens[bad[:5]]}, first byte "
                           f"{buf[offs[bad[:5]].astype(np.int64)]}: restatement {got[bad[:5]]} "
                           f"reference {want[bad[:5]]}")
    return want


def assert_py_matches(buf, offs, lens, kind, want, rng, what, always=()):
    """py_oracle on PY_SAMPLE cases (and those of `always`)."""
    pick = set(rng.choice(offs.size, min(PY_SAMPLE, offs.size), replace=False).tolist())
    fn = py_oracle.payload_cksum if kind else py_oracle.ip_cksum
    for i in sorted(pick | set(always)):
        o, n = int(offs[i]), int(lens[i])
        got = fn(buf[o:o + max(n, 40 if kind else 0)].tobytes(), n)
        assert got == int(want[i]), f"{what}: py_oracle case {i} (len {n})"


# ---------------------------------------------------------------------------
# ip_cksum

@pytest.mark.parametrize("fill", ["random", "zeros", "ones"])
def test_ip_cksum_sweep(ref, fill):
    """Start phases 0..15 x lengths 0..130, 255..257, 511, 1471..1473, 9000,
    9001, 65534, 65535 over random bytes, an all-0x00 and an all-0xFF buffer
    (the two negative zeros: 0xFFFF for a zero sum, 0x0000 for a non-zero
    multiple of 0xFFFF)."""
    rng = np.random.default_rng(41)
    size = 65535 + 15 + 64
    buf = {"random": rng.integers(0, 256, size, dtype=np.uint8),
           "zeros": np.zeros(size, np.uint8), "ones": np.full(size, 0xFF, np.uint8)}[fill]
    offs, lens = refcases.ip_sweep()
    assert offs.size == 16 * 142
    want = assert_c_matches(ref, buf, offs, lens, 0, f"ip_cksum, {fill}")
    big = np.flatnonzero(lens >= 65534)[:4]  # a few of the 64 KiB ones, not 300
    small = np.flatnonzero(lens < 65534)
    pick = np.concatenate((small, big))
    assert_py_matches(buf, offs[pick], lens[pick], 0, want[pick], rng, f"ip_cksum, {fill}",
                      always=range(small.size, pick.size))
    if fill == "zeros":
        assert (want == 0xFFFF).all()
    if fill == "ones":
        # len 0 sums nothing; an odd len ends in a lone 0x00FF
        assert (want[(lens > 0) & (lens % 2 == 0)] == 0x0000).all()
        assert (want[lens == 0] == 0xFFFF).all()


# ---------------------------------------------------------------------------
# payload_cksum, structured inputs

@pytest.fixture(scope="module")
def wild_packets():
    return random_packets(np.random.default_rng(42), 5000, max_payload=1472, wild=True)


@pytest.mark.parametrize("align,lead", [(1, 7), (2, 14), (16, 0)])
def test_payload_cksum_wild_packets(ref, wild_packets, align, lead):
    """5000 packets with IPv4 options, bad total lengths and any IPv6 next
    header, at three packings -- and the same packets with len redrawn in
    [hl, len]."""
    rng = np.random.default_rng(43 + align)
    buf, offs, lens = pack(wild_packets, align=align, lead=lead)
    assert_payload_domain(buf, offs, lens, 5000)
    want = assert_c_matches(ref, buf, offs, lens, 1, "wild packets")
    assert_py_matches(buf, offs, lens, 1, want, rng, "wild packets")
    short = refcases.redraw_lens(buf, offs, lens, rng)
    assert_payload_domain(buf, offs, short, 5000)
    assert (short < lens).sum() > 4000
    want = assert_c_matches(ref, buf, offs, short, 1, "wild packets, len redrawn")
    assert_py_matches(buf, offs, short, 1, want, rng, "wild packets, len redrawn")


def test_payload_cksum_ipv6_next_hdr_wrap(ref):
    """next_hdr << 24 added into a uint32 that wraps: all-0xFF payloads of
    60000, 65000 and 65487 bytes x next_hdr 17, 58, 128, 200, 255."""
    rng = np.random.default_rng(44)
    pkts = refcases.ipv6_wrap_packets(rng)
    buf, offs, lens = pack(pkts, align=1, lead=5)
    assert_payload_domain(buf, offs, lens, 15)
    wraps = [(pkt[6] << 24) + py_oracle.word_sum(pkt[8:40]) + py_oracle.word_sum(pkt[4:6])
             + py_oracle.word_sum(pkt[40:ln]) >= 1 << 32 for pkt, ln in pkts]
    assert any(wraps) and not all(wraps)  # the wrap happens in some, not in others
    want = assert_c_matches(ref, buf, offs, lens, 1, "IPv6 next_hdr wrap")
    assert_py_matches(buf, offs, lens, 1, want, rng, "IPv6 next_hdr wrap")


def test_payload_cksum_ipv4_total_length_below_header(ref):
    """IPv4 total length < hl: bswap16(bswap16(ip->len) - hl) wraps in 16
    bits.  Every total length 0..hl-1 for every IHL 5..15."""
    rng = np.random.default_rng(45)
    pkts = refcases.ipv4_totlen_wrap_packets(rng)
    buf, offs, lens = pack(pkts, align=1, lead=1)
    assert_payload_domain(buf, offs, lens, sum(4 * ihl for ihl in range(5, 16)))
    want = assert_c_matches(ref, buf, offs, lens, 1, "IPv4 total length < hl")
    assert_py_matches(buf, offs, lens, 1, want, rng, "IPv4 total length < hl")


def test_payload_cksum_every_version_and_ihl_nibble(ref):
    """Every first byte 0x00..0xFF, with len == hl and with a body: any
    version nibble but 4 is summed as IPv6, IPv4 with any IHL (IHL < 5 counts
    src / dst twice, IHL 0 sums the whole packet as payload)."""
    rng = np.random.default_rng(46)
    pkts = refcases.nibble_grid_packets(rng, bodies=(0, None, 1400))
    buf, offs, lens = pack(pkts, align=1, lead=3)
    assert_payload_domain(buf, offs, lens, 256 * 3)
    assert set(buf[offs.astype(np.int64)].tolist()) == set(range(256))
    want = assert_c_matches(ref, buf, offs, lens, 1, "version x IHL nibbles")
    assert_py_matches(buf, offs, lens, 1, want, rng, "version x IHL nibbles")


# ---------------------------------------------------------------------------
# payload_cksum, unstructured inputs

def test_payload_cksum_random_bytes(ref):
    """20000 cases of random bytes under a random first byte, len = hl +
    U[0, 2000), and one at len 65535."""
    rng = np.random.default_rng(47)
    buf, offs, lens = refcases.random_byte_cases(rng, 20000)
    assert_payload_domain(buf, offs, lens, 20001)
    assert lens[-1] == 65535
    v4 = buf[offs.astype(np.int64)] >> 4 == 4
    assert 800 < v4.sum() < 1700 and ((buf[offs.astype(np.int64)] & 15)[v4] < 5).any()
    want = assert_c_matches(ref, buf, offs, lens, 1, "random bytes")
    assert_py_matches(buf, offs, lens, 1, want, rng, "random bytes", always=[20000])


# ---------------------------------------------------------------------------
# The two checksum decisions of the RX chain, and the TX model's two values.

RX_CKSUM_CASES = ("ok4", "ok6", "ok4opt", "mf", "nocksum", "badudp", "badip", "ulen_big",
                  "ulen_small")
RX_CKSUM_VERDICTS = (py_oracle.RX_OK, py_oracle.RX_OK_NO_CKSUM, py_oracle.RX_BAD_UDP_CKSUM,
                     py_oracle.RX_BAD_IP_CKSUM)


def ref_rx_verdict(ref, frame: bytes) -> int:
    """The verdict of a frame that reached the checksum decisions, from the
    reference's two functions (the fields as ip4_rx / udp_rx read them)."""
    ip = frame[14:]
    v4 = frame[12:14] == b"\x08\x00"
    hl = (ip[0] & 0x0F) * 4 if v4 else 40
    if v4 and ref.ip_cksum(ip, hl) != 0:
        return py_oracle.RX_BAD_IP_CKSUM
    ip_plen = ((((ip[2] << 8) | ip[3]) - hl) & 0xFFFF) if v4 else (ip[4] << 8) | ip[5]
    if ip[hl + 6] == 0 and ip[hl + 7] == 0:
        return py_oracle.RX_OK_NO_CKSUM
    udp_len = min((ip[hl + 4] << 8) | ip[hl + 5], ip_plen)
    return py_oracle.RX_BAD_UDP_CKSUM if ref.payload_cksum(ip, udp_len + hl) != 0 \
        else py_oracle.RX_OK


def test_rx_checksum_decisions_are_the_references(ref):
    """The RX chain stays a restatement; wherever the oracle's verdict is one
    of the four that a checksum decides, the reference's ip_cksum over the
    header and payload_cksum over min(udp_len, ip_plen) + hl give the same
    verdict.  All frames of every case are in scope but badip's, where a
    flipped header bit may make a version / fragment / protocol case of the
    frame: at most 10 % of those."""
    rng = np.random.default_rng(48)
    per_case = 220
    frames = rx_ring(rng, per_case * len(RX_CKSUM_CASES), cases=RX_CKSUM_CASES, max_payload=700)
    buf, offs, lens = pack(frames, align=1, lead=3)
    verdict = c_oracle.rx_verdict_ragged(buf, offs, lens)
    scope = np.isin(verdict, RX_CKSUM_VERDICTS)
    case = np.arange(offs.size) % len(RX_CKSUM_CASES)
    for k, name in enumerate(RX_CKSUM_CASES):
        out = int((~scope & (case == k)).sum())
        print(f"{name}: {out} of {per_case} out of scope")
        assert out <= (per_case // 10 if name == "badip" else 0), name
    assert set(np.unique(verdict[scope]).tolist()) == set(RX_CKSUM_VERDICTS)
    b = buf.tobytes()
    for i in np.flatnonzero(scope).tolist():
        o, n = int(offs[i]), int(lens[i])
        assert ref_rx_verdict(ref, b[o:o + n]) == int(verdict[i]), (
            f"frame {i} ({RX_CKSUM_CASES[case[i]]}): oracle verdict {int(verdict[i])}")


@pytest.mark.parametrize("name", ["slots", "pack_1_0", "pack_1_5", "pack_2_14", "pack_16_3"])
def test_tx_model_values_are_the_references(ref, monkeypatch, name):
    """tests/tx_model.py's seal over the frames of test_seal_is_byte_exact,
    as it stands and with its two checksum calls answered by the reference:
    status, both values and the stored bytes are identical.  (Frames for which
    the model computes no checksum never reach the reference; where it does,
    len = hl + udp_len >= hl.)"""
    from test_gpu_tx import LAYOUTS, layout
    assert name in LAYOUTS
    buf, offs, lens = layout(name)
    ours = tx_model.Expect(buf, offs, lens)
    monkeypatch.setattr(tx_model, "c_oracle", ref)
    theirs = tx_model.Expect(buf, offs, lens)
    assert (ours.status == tx_model.SEALED).sum() > 100
    np.testing.assert_array_equal(ours.status, theirs.status)
    np.testing.assert_array_equal(ours.ip_hdr, theirs.ip_hdr)
    np.testing.assert_array_equal(ours.udp, theirs.udp)
    assert [s.stores for s in ours.seals] == [s.stores for s in theirs.seals]
    np.testing.assert_array_equal(ours.buf, theirs.buf)


def test_boundary_grid_checksum_decisions_are_the_references(ref):
    """The same over tests/rx_edges.py's grid, the frames that stand on the
    chain's thresholds: every frame whose verdict is one of the four a
    checksum decides -- none left out -- gets it from the reference's
    functions too (IHL < 5 and udp_len + hl < 20 included: len >= hl there)."""
    import rx_edges
    frames = rx_edges.grid()
    verdict = rx_edges.oracle_verdicts(frames)
    scope = np.flatnonzero(np.isin(verdict, RX_CKSUM_VERDICTS))
    assert set(verdict[scope].tolist()) == set(RX_CKSUM_VERDICTS) and scope.size > 1000
    for i in scope.tolist():
        fr, flen, tag = frames[i]
        assert ref_rx_verdict(ref, fr[:flen]) == int(verdict[i]), (
            f"{tag}: oracle verdict {int(verdict[i])}")


@pytest.mark.parametrize("zero_udp", [False, True])
def test_boundary_grid_tx_model_values_are_the_references(ref, monkeypatch, zero_udp):
    """tx_model's seal over the grid (fields garbled, as the GPU test hands it
    over) with its two checksum calls answered by the reference: identical."""
    import rx_edges
    buf, offs, lens = rx_edges.packed(rx_edges.garbled(rx_edges.grid()), phase=3)
    ours = tx_model.Expect(buf, offs, lens, zero_udp=zero_udp)
    monkeypatch.setattr(tx_model, "c_oracle", ref)
    theirs = tx_model.Expect(buf, offs, lens, zero_udp=zero_udp)
    assert (ours.status == (tx_model.SEALED_ZERO_UDP if zero_udp else tx_model.SEALED)).sum() > 500
    np.testing.assert_array_equal(ours.status, theirs.status)
    np.testing.assert_array_equal(ours.ip_hdr, theirs.ip_hdr)
    np.testing.assert_array_equal(ours.udp, theirs.udp)
    assert [s.stores for s in ours.seals] == [s.stores for s in theirs.seals]
    np.testing.assert_array_equal(ours.buf, theirs.buf)


# ---------------------------------------------------------------------------
# The strided grid (tests/strided_grid.py): what the GPU tests compare with.

def test_strided_grid_expectations_are_the_references(ref):
    """Every buffer of the strided grid at its largest n (the smaller n are
    prefixes of it): the ip, payload and header-checksum expectations the GPU
    tests use are what the reference's functions give on the same bytes; no
    case left out (every payload case has len >= hl: asserted per buffer)."""
    import strided_grid as sg
    groups = sg.groups(sg.grid())
    packets = 0
    for case in groups:
        buf, want = sg.buffer(case), sg.expect(case)
        offs, lens = case.offs, np.full(case.n, case.length, np.uint16)
        np.testing.assert_array_equal(ref.cksum_ragged(buf, offs, lens, kind=0), want["ip"],
                                      err_msg=f"ip {case[:4]}")
        if "payload" not in case.kinds:
            continue
        assert_payload_domain(buf, offs, lens, case.n)
        np.testing.assert_array_equal(ref.cksum_ragged(buf, offs, lens, kind=1), want["payload"],
                                      err_msg=f"payload {case[:4]}")
        np.testing.assert_array_equal(refcases.hdr_expect(buf, offs), want["hdr"],
                                      err_msg=f"hdr {case[:4]}")
        packets += case.n
    assert len(groups) == 2592 and packets > 300000


def test_strided_grid_short_headers_are_the_references(ref):
    """The IPv4 packets with 20 <= len < hl: the expected header checksums
    are the reference's ip_cksum(pkt, hl).  (Its payload_cksum is never
    called on them.)"""
    import strided_grid as sg
    cases = [c for c in sg.short_header_cases() if c.n == sg.N_SET[-1]]
    assert len(cases) == 135
    for case in cases:
        np.testing.assert_array_equal(refcases.hdr_expect(sg.short_buffer(case), case.offs),
                                      sg.short_expect(case), err_msg=str(case))
    pk = sg.short_packets()
    buf, offs, _ = pack(list(pk), align=1, lead=3)
    np.testing.assert_array_equal(refcases.hdr_expect(buf, offs), sg.header_checksums(buf, offs))


# ---------------------------------------------------------------------------
# The guard and the fixture.

def test_guard_refuses_len_below_header_length(monkeypatch):
    """payload_cksum with len < hl is a ~4 GiB read in the reference: the
    wrapper raises before anything is loaded or called.  (What the reference
    does there is not tested: it is a crash.)"""
    def no_call():
        raise AssertionError("the guard let a len < hl call through to the object")
    monkeypatch.setattr(ref_oracle, "load", no_call)
    v4 = np.zeros(64, np.uint8)
    v4[0] = 0x4F  # IPv4, IHL 15: hl = 60
    v6 = np.zeros(64, np.uint8)
    v6[0] = 0x60
    for pkt, ln in ((v4, 20), (v4, 59), (v6, 39), (v6, 0)):
        with pytest.raises(ValueError, match="header length"):
            ref_oracle.payload_cksum(pkt, ln)
        with pytest.raises(ValueError, match="header length"):
            ref_oracle.payload_cksum(pkt.tobytes(), ln)
        with pytest.raises(ValueError, match="header length"):
            ref_oracle.cksum_ragged(np.concatenate((v6, pkt)), np.array([0, 64], np.uint64),
                                    np.array([40, ln], np.uint16), kind=1)


def test_ref_fixture_matches_live_reference(ref):
    """tests/golden/ref_vectors.npz, the recorded results the GPU tests run
    against, is what the live object computes today."""
    g = np.load(refcases.REF_VECTORS)
    live = refcases.expects(g)
    assert set(live) == {k for k in g.files if k.endswith("_expect") or k == "tx_status"}
    for k, want in live.items():
        np.testing.assert_array_equal(g[k], want, err_msg=k)
    # what the fixture is there for is in it
    assert g["pl_len"].max() == 65535
    assert set(g["pl_blob"][g["pl_off"].astype(np.int64)].tolist()) >= set(range(256))
    assert (g["tx_status"] == tx_model.SEALED).sum() > 300
    assert refcases.REF_VECTORS.stat().st_size <= 461362  # the largest fixture so far
