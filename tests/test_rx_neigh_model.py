"""CPU tests of the RX neighbours' model (tests/rx_neigh_model.py) and cases:
the boundary grid's hand-stated expectations, the census of codes and causes
in every world the GPU tests use, the four known answers, the model's replies
read back through the RX verdict, the reply plan and the neighbour plan of the
other end, and -- where the reference's own checksum object is present -- its
verdict on every model advertisement."""
import numpy as np
import pytest

import rx_neigh_cases as cases
import rx_neigh_model as model
import rx_reply_cases as rc
import rx_reply_model as rmodel
from oracle import c_oracle, ref_oracle


@pytest.fixture(scope="module")
def grid():
    return cases.grid()


def test_grid_expectations(grid):
    for name, fr, act, eng, code in grid:
        assert model.plan(fr, act, eng) == code, name
        assert (model.build(fr, code, eng) is not None) == (code in model.REPLIES), name
        assert (model.record(fr, code) is not None) == (code in model.UPDATES), name


def test_grid_holds_both_sides_of_every_comparison(grid):
    names = {g[0] for g in grid}
    for pair in (("arp flen 42", "arp flen 41"), ("nsol flen 55", "nsol flen 54"),
                 ("nsol flen 78", "nsol flen 77"), ("nadv flen 78", "nadv flen 77"),
                 ("nsol flen 86", "nsol flen 85"), ("nsol ip6 len 24", "nsol ip6 len 23"),
                 ("nadv ip6 len 24", "nadv ip6 len 23"), ("nsol option 0101", "nsol option 0001"),
                 ("nsol option 0100", "nsol option 0201"), ("nadv option 0101", "nadv option 0201"),
                 ("arp hln 5 off by one", "arp hln 7 off by one"),
                 ("arp pln 3 off by one", "arp pln 5 off by one"),
                 ("arp hrd off by one", "arp pro off by one"),
                 ("arp op 0000", "arp op 0001"), ("arp op 0002", "arp op 0003"),
                 ("arp op 0100", "arp tpa second address"),
                 ("arp tpa bcast", "arp tpa 255.255.255.255"), ("arp, no af-4 entry", "arp flen 60"),
                 ("nsol target second address", "nsol target snma"),
                 ("nsol target = an IPv4 entry's bytes", "nsol target other"),
                 ("host on an echo4 frame", "host on an echo6 frame"),
                 ("ethertype 81 00", "ethertype 06 08"), ("flen 13", "flen 14, arp")):
        assert set(pair) <= names, pair
    stale = {g[2] for g in grid if g[0].startswith("arp, action")}
    assert stale >= set(rmodel.ALL_ACTIONS) - {rmodel.HOST} and {31, 255} <= stale
    assert {g[4] for g in grid} == set(model.ALL_ACTIONS)


def mac_of(fr, code):
    return model.record(fr, code)[2]


def test_the_option_rule_on_both_sides(grid):
    by = {g[0]: g for g in grid}
    for kind, code in (("nsol", model.NADV), ("nadv", model.UPDATE6)):
        assert mac_of(by[f"{kind} option 0101"][1], code) == cases.OPT_MAC
        for o in ("0001", "0100", "0201"):
            assert mac_of(by[f"{kind} option {o}"][1], code) == rc.PEER_MAC, o
        assert mac_of(by[f"{kind} ip6 len 24"][1], code) == cases.OPT_MAC
        assert mac_of(by[f"{kind} ip6 len 23"][1], code) == rc.PEER_MAC
    assert mac_of(by["nsol flen 86"][1], model.NADV) == cases.OPT_MAC
    assert mac_of(by["nsol flen 85"][1], model.NADV) == rc.PEER_MAC


def world_expect(name, eng):
    seed, n = cases.WORLDS[name]
    frames = cases.world(seed, n)
    buf, offs, lens = cases.layout(name, frames, seed)
    return frames, model.Expect(buf, offs, lens, cases.actions_of(frames, eng), eng)


@pytest.mark.parametrize("name", list(cases.WORLDS))
def test_census_at_least_ten_of_every_code_and_cause(name):
    _, ex = world_expect(name, rc.engine_table())
    c = ex.census()
    assert set(c) == set(cases.CENSUS)
    for key in cases.CENSUS:
        assert c[key] >= 10, key
    _, ex = world_expect(name, rc.engine_table(v4=0))
    assert ex.census()[(model.NONE, "no ip4")] >= 10
    assert len(ex.rlist) >= 10 and len(ex.ulist) >= 20


def test_known_answers():
    eng = rc.engine_table()
    nsol, arp = bytes.fromhex(cases.NSOL_HEX), bytes.fromhex(cases.ARP_HEX)
    assert nsol == cases.nd(135, rc.A6[0], opt=b"\x01\x01" + rc.PEER_MAC)
    assert arp == cases.arp(tpa=rc.A4[1])
    assert model.plan(nsol, model.HOST, eng) == model.NADV
    assert model.plan(arp, model.HOST, eng) == model.ARP_IS_AT
    nadv, is_at = model.build(nsol, model.NADV, eng), model.build(arp, model.ARP_IS_AT, eng)
    assert nadv.hex() == cases.NADV_HEX and is_at.hex() == cases.IS_AT_HEX
    assert c_oracle.payload_cksum(nadv[14:], 72) == 0
    assert model.record(nsol, model.NADV) == (6, model.NADV, rc.PEER_MAC, rc.PEER6)
    assert model.record(arp, model.ARP_IS_AT) == (4, model.ARP_IS_AT, rc.PEER_MAC, rc.PEER4 + bytes(12))


def all_replies():
    """(request, code, reply) of the grid, one world and the peer's requests."""
    eng = rc.engine_table()
    out = [(fr, code, model.build(fr, code, e)) for _, fr, _, e, code in cases.grid()
           if code in model.REPLIES]
    frames, ex = world_expect("slots", eng)
    out += [(fr, int(c), model.build(fr, int(c), eng)) for (fr, _, _), c in zip(frames, ex.nact)
            if c in model.REPLIES]
    out += [(fr, model.plan(fr, model.HOST, eng), model.build(fr, model.plan(fr, model.HOST, eng), eng))
            for fr, _, _ in cases.peer_requests()]
    return out


def test_advertisement_checksums_are_the_references():
    if not ref_oracle.available():
        pytest.skip("no oracle/_ref/libwc_ref.so and no reference tree (WC_REFERENCE_DIR) to "
                    "build it from")
    k = 0
    for fr, code, reply in all_replies():
        if code == model.NADV:
            assert len(reply) == 86 and ref_oracle.payload_cksum(reply[14:], 72) == 0
            k += 1
    assert k > 50


def test_reply_fields():
    for fr, code, reply in all_replies():
        assert reply[6:12] == rc.MAC
        if code == model.ARP_IS_AT:
            assert len(reply) == 42 and reply[0:6] == fr[22:28] == reply[32:38]
            assert reply[12:22] == bytes.fromhex("08060001080006040002")
            assert reply[22:28] == rc.MAC and reply[28:32] == fr[38:42] and reply[38:42] == fr[28:32]
        else:
            assert len(reply) == 86 and reply[0:6] == fr[6:12]
            assert reply[12:22] == bytes.fromhex("86dd6000000000203aff")
            assert reply[22:38] == rc.A6[0] and reply[38:54] == fr[22:38]
            assert reply[54:56] == b"\x88\x00" and reply[58:62] == b"\x60\x00\x00\x00"
            assert reply[62:78] == fr[62:78] and reply[78:86] == b"\x02\x01" + rc.MAC
            assert c_oracle.payload_cksum(reply[14:], 72) == 0


def test_replies_are_updates_with_our_address_and_mac_at_the_other_end():
    eng, peer = rc.engine_table(), rc.peer_table()
    seen = set()
    for fr, _, _ in cases.peer_requests():
        code = model.plan(fr, model.HOST, eng)
        reply = model.build(fr, code, eng)
        v = c_oracle.rx_verdict(reply, len(reply))
        act, _ = rmodel.plan(reply, v, None, peer, 2048)
        assert act == rmodel.HOST
        back = model.plan(reply, act, peer)
        if code == model.ARP_IS_AT:
            assert back == model.UPDATE4
            assert model.record(reply, back) == (4, back, rc.MAC, fr[38:42] + bytes(12))
        else:
            assert back == model.UPDATE6
            assert model.record(reply, back) == (6, back, rc.MAC, fr[62:78])
        seen.add(code)
    assert seen == set(model.REPLIES)


def test_a_damaged_advertisement_is_a_bad_checksum_at_the_other_end():
    eng, peer = rc.engine_table(), rc.peer_table()
    reply = model.build(bytes.fromhex(cases.NSOL_HEX), model.NADV, eng)
    bad = rc.flip(reply, 85)
    v = c_oracle.rx_verdict(bad, len(bad))
    assert rmodel.plan(bad, v, None, peer, 2048)[0] == rmodel.ICMP_BAD_CKSUM
    assert model.plan(bad, rmodel.ICMP_BAD_CKSUM, peer) == model.NONE


def test_records_come_out_in_ring_order():
    _, ex = world_expect("packed", rc.engine_table())
    assert (np.diff(ex.ulist.astype(np.int64)) > 0).all() and set(ex.rlist) <= set(ex.ulist)
    upd = ex.updates(len(ex.ulist) + 3).view(model.UPDATE).reshape(-1)
    assert (upd["af"][:len(ex.ulist)] != 0).all() and not upd["af"][len(ex.ulist):].any()
    assert (upd["action"][:len(ex.ulist)] == ex.nact[ex.ulist]).all()
