"""CPU test of the lines the TX build kernel and wc_tx_build_host share
(warpcore_amd/csrc/wc_tx_build.h), compiled for the host alone
(tests/c/tx_build_words.cpp): check chain, header bytes, both checksum values
and the stores at every 16-byte phase against tests/tx_build_model.py.  The
program itself refuses a store that is misaligned or leaves the header bytes."""
import struct
import subprocess

import numpy as np
import pytest

import cprog
import tx_build_cases as cases
import tx_build_model as model



@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return cprog.build_words("tx_build_words", tmp_path_factory.mktemp("txb"))


def run(exe, tmp_path, items):
    """items: (sock entry or None, dst entry or None, desc, slot_bytes, zero_udp,
    phase, payload) -> [(status, flen, ip_hdr, udp, region bytes)]."""
    blob = bytearray()
    for sk, ds, d, slot, zero, phase, pay in items:
        blob += sk.tobytes() if sk is not None else bytes(52)
        blob += ds.tobytes() if ds is not None else bytes(24)
        blob += d.tobytes()
        blob += struct.pack("<6I", sk is not None, ds is not None, slot, zero, phase, len(pay))
        blob += pay
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(bytes(blob))
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = dst.read_bytes()
    assert len(raw) == len(items) * 144
    return [struct.unpack("<4I", raw[i:i + 16]) + (raw[i + 16:i + 144],)
            for i in range(0, len(raw), 144)]


@pytest.mark.parametrize("zero_udp", [False, True])
def test_words_and_stores_every_phase(exe, tmp_path, zero_udp):
    rng = np.random.default_rng(77 + zero_udp)
    socks, dsts = cases.socks_table(rng, 8), cases.dsts_table(rng, 3)
    lens = (0, 1, 2, 7, 16, 33, 64, 129, 1472)
    items, want = [], []
    for phase in range(16):
        descs = cases.descs_for(rng, 48, 8, 3, data_lens=lens)
        for d in descs:
            pay = rng.integers(0, 256, int(d["data_len"]), dtype=np.uint8).tobytes()
            sk = socks[int(d["sock"])]
            items.append((sk, dsts[int(d["dst"])], d, 2048, zero_udp, phase, pay))
            fr, ipck, udpck = model.build_frame(d, socks, dsts, pay, zero_udp)
            hb = model.hdr_len(int(sk["af"]))
            region = bytearray(b"\xa5" * 128)
            region[16 + phase:16 + phase + hb] = fr[:hb]
            want.append((int(zero_udp), hb + len(pay), ipck, udpck, bytes(region)))
    got = run(exe, tmp_path, items)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g == w, f"case {i} (phase {i // 48}, desc {items[i][2]})"


def test_computed_zero_checksum_stays_zero(exe, tmp_path):
    rng = np.random.default_rng(5)
    socks, dsts = cases.socks_table(rng, 8), cases.dsts_table(rng, 1)
    for s in (2, 3):  # a connected IPv4 and IPv6 socket
        d = cases.descs_for(rng, 1, 8, 1, data_lens=(64,))[0]
        d["sock"] = s
        pay = bytearray(64)
        _, _, c = model.build_frame(d, socks, dsts, bytes(pay))
        pay[10:12] = bytes((c & 0xFF, c >> 8))  # a zero payload word takes the complement
        fr, _, c0 = model.build_frame(d, socks, dsts, bytes(pay))
        assert c0 == 0
        (st, flen, _, udp, region), = run(exe, tmp_path, [(socks[s], None, d, 2048, 0, 1,
                                                            bytes(pay))])
        hb = model.hdr_len(int(socks[s]["af"]))
        assert (st, udp) == (model.SEALED, 0) and region[17:17 + hb] == fr[:hb]
        assert region[17 + hb - 2:17 + hb] == b"\x00\x00"


def test_check_chain_order(exe, tmp_path):
    rng = np.random.default_rng(6)
    socks, dsts = cases.socks_table(rng, 8), cases.dsts_table(rng, 2)
    bad_af = socks[0].copy()
    bad_af["af"] = 5

    def one(sk, ds, slot=2048, **kw):
        d = np.zeros(1, model.DESC)[0]
        d["data_len"] = 100
        for k, v in kw.items():
            d[k] = v
        (st, flen, ipck, udp, region), = run(exe, tmp_path, [(sk, ds, d, slot, 0, 0,
                                                             bytes(int(d["data_len"])))])
        if st > model.SEALED_ZERO_UDP:
            assert (flen, ipck, udp) == (0, 0, 0) and region == b"\xa5" * 128
        return st

    assert one(socks[0], dsts[0]) == model.SEALED
    assert one(None, dsts[0]) == model.MALFORMED                      # sock >= ns
    assert one(bad_af, dsts[0]) == model.MALFORMED                    # af 5
    assert one(socks[0], None) == model.MALFORMED                     # unconnected, dst >= ndst
    assert one(socks[2], None) == model.SEALED                        # connected: dst ignored
    assert one(socks[0], dsts[0], slot=141) == model.TRUNCATED        # 142-byte frame
    assert one(socks[0], dsts[0], slot=142) == model.SEALED
    assert one(socks[1], dsts[0], slot=161) == model.TRUNCATED        # IPv6: 162 bytes
    assert one(socks[2], None, slot=1 << 16, data_len=65493) == model.SEALED     # 65535 bytes
    assert one(socks[2], None, slot=1 << 16, data_len=65494) == model.MALFORMED
    assert one(socks[3], None, slot=1 << 16, data_len=65473) == model.SEALED     # IPv6
    assert one(socks[3], None, slot=1 << 16, data_len=65474) == model.MALFORMED
    assert one(socks[2], None, slot=100, data_len=65494) == model.MALFORMED      # before TRUNCATED
    assert one(None, None, slot=0) == model.MALFORMED                 # two failures: the first
    assert one(socks[0], None, slot=0) == model.MALFORMED
