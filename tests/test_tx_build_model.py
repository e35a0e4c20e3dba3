"""CPU tests of the tests' own model of the TX build (tests/tx_build_model.py):
a frame it builds is one the RX side accepts -- the C oracle's verdict, the
reference's own checksum object where it exists, and the delivery record that
udp_rx would fill give back what the descriptor asked for."""
import functools

import numpy as np
import pytest

import rx_deliver_model
import tx_build_cases as cases
import tx_build_model as model
from oracle import c_oracle, ref_oracle

RX_OK, RX_OK_NO_CKSUM = 0, 1


@functools.lru_cache(maxsize=None)
def built(zero_udp: bool):
    """(frames, descs, socks, dsts): 96 frames over all eight socket kinds and
    every TOS value, the issue's data lengths."""
    rng = np.random.default_rng(31 + zero_udp)
    socks, dsts = cases.socks_table(rng, 8), cases.dsts_table(rng, 5)
    descs = cases.descs_for(rng, 96, 8, 5, data_lens=cases.DATA_LENS)
    frames = []
    for d in descs:
        pay = rng.integers(0, 256, int(d["data_len"]), dtype=np.uint8).tobytes()
        frames.append(model.build_frame(d, socks, dsts, pay, zero_udp)[0])
    return frames, descs, socks, dsts


@pytest.mark.parametrize("zero_udp", [False, True])
def test_built_frames_pass_the_rx_checks(zero_udp):
    frames, descs, socks, _ = built(zero_udp)
    buf = np.frombuffer(b"".join(frames), np.uint8)
    lens = np.array([len(f) for f in frames], np.uint16)
    offs = (np.cumsum(lens.astype(np.uint64)) - lens).astype(np.uint64)
    got = c_oracle.rx_verdict_ragged(buf, offs, lens)
    if zero_udp:
        assert (got == RX_OK_NO_CKSUM).all()
    else:
        # (a computed 0 is stored as 0 and read as "no checksum")
        zero = np.array([f[-int(d["data_len"]) - 2:len(f) - int(d["data_len"])] == b"\x00\x00"
                         for f, d in zip(frames, descs)])
        np.testing.assert_array_equal(got, np.where(zero, RX_OK_NO_CKSUM, RX_OK))
        assert (got == RX_OK).sum() >= 90
    for f, d in zip(frames, descs):
        af = int(socks[int(d["sock"])]["af"])
        assert len(f) == model.hdr_len(af) + int(d["data_len"])


@pytest.mark.skipif(not ref_oracle.available(), reason="no reference checksum object")
def test_reference_checksums_of_built_frames_are_zero():
    frames, descs, socks, _ = built(False)
    for f, d in zip(frames, descs):
        ip = f[14:]
        if int(socks[int(d["sock"])]["af"]) == 4:
            assert ref_oracle.ip_cksum(ip[:20]) == 0
        assert ref_oracle.payload_cksum(ip, len(ip)) == 0


@pytest.mark.parametrize("zero_udp", [False, True])
def test_delivery_record_gives_back_the_descriptor(zero_udp):
    frames, descs, socks, dsts = built(zero_udp)
    seen_v6_dropped_class = 0
    for f, d in zip(frames, descs):
        r = rx_deliver_model.record_of(f, len(f))
        sk = socks[int(d["sock"])]
        af, fl, tos = int(sk["af"]), int(sk["flags"]), int(d["tos"])
        conn = fl & model.SOCK_CONNECTED
        dport = int(sk["rport"]) if conn else int(dsts[int(d["dst"])]["port"])
        ecn_default = (tos & 3) == 0 and fl & model.SOCK_ECN
        if af == 4:  # ip4->tos
            want_tos = tos | (2 if ecn_default else 0)
        else:
            # ip6_tos reads the class and ECN bits of bytes 0..1 (ip6.h:77-81).
            # Without ECN bits in v->flags mk_ip6_hdr writes neither the class
            # (ip6.c:133) nor -- the default ECT0 goes to bit 21, byte 2 -- any
            # bit that ip6_tos reads: 0.
            want_tos = tos if tos & 3 else 0
            seen_v6_dropped_class += tos == 0xB8
        assert (int(r["af"]), int(r["data_len"]), int(r["sport"]), int(r["dport"]),
                int(r["ttl"]), int(r["tos"])) == \
            (af, int(d["data_len"]), int(sk["lport"]), dport, 255, want_tos), (d, sk)
        assert int(r["data_off"]) == model.hdr_len(af)
    assert seen_v6_dropped_class >= 2  # the quirk is pinned: class 0xb8 in, 0 out
