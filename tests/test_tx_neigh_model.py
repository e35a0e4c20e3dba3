"""CPU tests of the TX neighbours' model (tests/tx_neigh_model.py) and cases:
the two known-answer frames, the cache, resolve and hold rules, the model's
solicitations read back through the RX verdict, the reply plan and the
neighbour plan of the other end, that end's reply fed back into the cache model
-- and, where the reference's own checksum object is present, its verdict on
every model solicitation.  arp.c has no checksum to pin."""
import numpy as np
import pytest

import rx_neigh_model as nmodel
import rx_reply_cases as rc
import rx_reply_model as rmodel
import tx_neigh_cases as cases
import tx_neigh_model as model
from oracle import c_oracle, ref_oracle


def test_known_answers():
    eng = rc.engine_table()
    arp, nsol = model.solicit(4, cases.PEER4, eng), model.solicit(6, cases.PEER6, eng)
    assert arp.hex() == cases.ARP_WHO_HAS_HEX and len(arp) == model.ARP_LEN
    assert nsol.hex() == cases.NSOL_HEX and len(nsol) == model.NSOL_LEN
    assert c_oracle.payload_cksum(nsol[14:], 72) == 0
    # the fields, one by one
    assert arp[0:6] == model.BCAST and arp[6:12] == rc.MAC == arp[22:28]
    assert arp[12:22] == bytes.fromhex("08060001080006040001")
    assert arp[28:32] == rc.A4[0] and arp[32:38] == bytes(6) and arp[38:42] == cases.PEER4
    assert nsol[0:6] == b"\x33\x33" + cases.PEER6[12:16] and nsol[6:12] == rc.MAC
    assert nsol[12:22] == bytes.fromhex("86dd6000000000203aff") and nsol[22:38] == rc.A6[0]
    assert nsol[38:54] == bytes.fromhex("ff0200000000000000000001ff") + cases.PEER6[13:16]
    assert nsol[54:56] == b"\x87\x00" and nsol[58:62] == b"\x60\x00\x00\x00"
    assert nsol[62:78] == cases.PEER6 and nsol[78:86] == b"\x01\x01" + rc.MAC


def test_no_frame_without_an_address_of_the_family():
    assert model.solicit(4, cases.PEER4, rc.engine_table(v4=0)) is None
    assert model.solicit(6, cases.PEER6, rc.engine_table(v6=0)) is None
    assert model.solicit(6, cases.PEER6, rc.engine_table(v4=0)) is not None
    assert model.solicit(4, cases.PEER4, rc.engine_table(v6=0)) is not None
    for af in (0, 5, 7, 255):
        assert model.solicit(af, cases.PEER6, rc.engine_table()) is None


def all_solicitations():
    eng = rc.engine_table()
    out = [(af, a, model.solicit(af, a, eng), eng) for af, a in cases.keys(120) + cases.lookalikes()]
    rng = np.random.default_rng(1)
    for _ in range(60):
        e = rc.engine_table(rng=rng)
        a = rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
        out.append((6, a, model.solicit(6, a, e), e))
    return out


def test_solicitation_checksums_are_the_references():
    if not ref_oracle.available():
        pytest.skip("no oracle/_ref/libwc_ref.so and no reference tree (WC_REFERENCE_DIR) to "
                    "build it from")
    k = 0
    for af, _, fr, _ in all_solicitations():
        if af == 6:
            assert len(fr) == 86
            zeroed = fr[:56] + b"\x00\x00" + fr[58:]
            assert rmodel._le16(ref_oracle.payload_cksum(zeroed[14:], 72)) == fr[56:58]
            assert ref_oracle.payload_cksum(fr[14:], 72) == 0
            k += 1
    assert k > 100


def test_cache_rules():
    a = bytes((10, 9, 8, 7))
    upd = model.records([(4, b"\x02" * 6, a + b"\x55" * 12), (6, b"\x03" * 6, a + bytes(12)),
                         (0, b"\x04" * 6, a), (7, b"\x05" * 6, a), (4, b"\x06" * 6, a + b"\x66" * 12)])
    cache = {}
    assert model.apply(cache, upd, 5, 5) == 1
    assert cache == {(4, a): b"\x06" * 6, (6, a + bytes(12)): b"\x03" * 6}
    cache = {}
    assert model.apply(cache, upd, 9, 4) == 1 and cache[(4, a)] == b"\x02" * 6  # m below the count
    cache = {}
    assert model.apply(cache, upd, 1, 5) == 0 and len(cache) == 1               # count below m
    assert model.find(cache, 4, a + b"\x77" * 12) == b"\x02" * 6
    assert model.find(cache, 6, a + bytes(12)) == model.BCAST


def test_resolve_rules():
    ks = cases.keys(6)
    cache = {model.key(af, a): bytes((2, 0, 0, 0, 0, i)) for i, (af, a) in enumerate(ks)}
    cache[model.key(*ks[5])] = model.BCAST  # cached, broadcast: unresolved
    miss4, miss6 = (4, cases.addr4(500) + bytes(12)), (6, cases.addr6(500))
    order = [ks[0], miss4, ks[1], miss6, miss4, ks[5], (7, ks[0][1]), miss6, ks[5], ks[0]]
    rng = np.random.default_rng(0)
    dsts = cases.dst_table([(a, 1000 + i) for i, (_, a) in enumerate(order)], rng)
    afs = np.array([af for af, _ in order], np.uint8)
    state, after, lst = model.resolve(cache, dsts, afs)
    M = model
    assert state.tolist() == [M.READY, M.MISS, M.READY, M.MISS, M.MISS_DUP, M.MISS, M.BAD_AF,
                              M.MISS_DUP, M.MISS_DUP, M.READY]
    assert lst.tolist() == [1, 3, 5]
    assert (after["addr"] == dsts["addr"]).all() and (after["port"] == dsts["port"]).all()
    assert bytes(after["dmac"][0]) == bytes((2, 0, 0, 0, 0, 0)) == bytes(after["dmac"][9])
    assert bytes(after["dmac"][6]) == bytes(dsts["dmac"][6])  # BAD_AF: untouched
    for k in (1, 3, 4, 5, 7, 8):
        assert bytes(after["dmac"][k]) == model.BCAST
    assert all((M.MASK_SOLICIT >> int(s)) & 1 == (s == M.MISS) for s in state)
    assert all((M.MASK_MISS >> int(s)) & 1 == (s in (M.MISS, M.MISS_DUP)) for s in state)


def test_hold_grid():
    g = cases.hold_grid()
    socks = cases.socks_table()
    afs = np.array([a for a, _ in cases.HOLD_DSTS], np.uint8)
    state = np.array([s for _, s in cases.HOLD_DSTS], np.uint8)
    hold, lst = model.hold(cases.descs_of([(s, t) for _, s, t, _ in g]), socks, state, afs)
    for (name, _, _, code), h in zip(g, hold):
        assert h == code, name
    assert {c for _, _, _, c in g} == {model.TH_READY, model.TH_MALFORMED, model.TH_HELD}
    assert lst.tolist() == [i for i, x in enumerate(g) if x[3] == model.TH_HELD]
    # without a destination table every unconnected frame is malformed
    hold, lst = model.hold(cases.descs_of([(0, 0), (2, 0)]), socks, None, None)
    assert hold.tolist() == [model.TH_MALFORMED, model.TH_READY] and lst.size == 0


def test_each_solicitation_is_answered_and_the_answer_resolves_the_address():
    """Solicitation -> the target's RX path (HOST, then ARP_IS_AT / NADV) -> its
    reply -> our RX path (UPDATE4 / UPDATE6) -> the cache model -> READY."""
    eng = rc.engine_table()
    cache = {}
    for mac, a4, a6 in cases.peers():
        peer = cases.peer_engine(mac, a4, a6)
        for af, a in ((4, a4), (6, a6)):
            fr = model.solicit(af, a, eng)
            v = c_oracle.rx_verdict(fr, len(fr))
            act, _ = rmodel.plan(fr, v, None, peer, 2048)
            assert act == rmodel.HOST
            code = nmodel.plan(fr, act, peer)
            assert code == (nmodel.ARP_IS_AT if af == 4 else nmodel.NADV)
            # the peer learns us from the request
            assert nmodel.record(fr, code)[2:] == (rc.MAC, (rc.A4[0] + bytes(12)) if af == 4 else rc.A6[0])
            reply = nmodel.build(fr, code, peer)
            v = c_oracle.rx_verdict(reply, len(reply))
            act, _ = rmodel.plan(reply, v, None, eng, 2048)
            assert act == rmodel.HOST
            back = nmodel.plan(reply, act, eng)
            assert back == (nmodel.UPDATE4 if af == 4 else nmodel.UPDATE6)
            rec = np.frombuffer(nmodel.record_bytes(reply, back), model.UPDATE)
            assert model.apply(cache, rec, 1, 1) == 0
            assert model.find(cache, af, a) == mac
    dsts = cases.dst_table([(a4, 7) for _, a4, _ in cases.peers()] + [(a6, 7) for _, _, a6 in cases.peers()])
    afs = np.array([4] * 12 + [6] * 12, np.uint8)
    state, after, lst = model.resolve(cache, dsts, afs)
    assert not state.any() and lst.size == 0
    assert [bytes(m) for m in after["dmac"]] == [p[0] for p in cases.peers()] * 2


def test_a_solicitation_for_another_host_is_not_answered():
    eng = rc.engine_table()
    mac, a4, a6 = cases.peers()[0]
    other = cases.peer_engine(*cases.peers()[1])
    for af, a in ((4, a4), (6, a6)):
        fr = model.solicit(af, a, eng)
        v = c_oracle.rx_verdict(fr, len(fr))
        act, _ = rmodel.plan(fr, v, None, other, 2048)
        assert nmodel.plan(fr, act, other) not in nmodel.REPLIES
