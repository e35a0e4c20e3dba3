"""CPU tests of the RX replies' model (tests/rx_reply_model.py) and cases: the
boundary grid's hand-stated expectations, the census of action codes in the
grid and in every world the GPU tests use, the model's replies read back
through the RX verdict and the plan of the other end, and -- where the
reference's own checksum object is present -- every checksum decision and
value of the model against it."""
import numpy as np
import pytest

import rx_reply_cases as cases
import rx_reply_model as model
from oracle import c_oracle, ref_oracle

NOT_UDP = model.RX_NOT_UDP


@pytest.fixture(scope="module")
def grid():
    return cases.grid()


def planned(frames, socks, eng, slot):
    v = cases.verdicts_of(frames)
    return [model.plan(fr, int(v[i]), None if socks is None else int(socks[i]), eng, slot)
            for i, (fr, _) in enumerate(frames)]


def test_grid_expectations(grid):
    for name, fr, sock, eng, slot, act, ln in grid:
        got = model.plan(fr, c_oracle.rx_verdict(fr, len(fr)), sock, eng, slot)
        assert got == (act, ln), name
        r = model.build(fr, act, eng) if act in model.REPLIES else None
        assert (len(r) if r else 0) == ln, name


def test_grid_holds_both_sides_of_every_comparison(grid):
    names = {g[0] for g in grid}
    for pair in (("echo4 ip_len = hl + 8", "echo4 ip_len = hl + 7"),
                 ("echo6 ip6_len = 8", "echo6 ip6_len = 7"),
                 ("echo4 ip_len = the frame's", "echo4 ip_len one past the frame"),
                 ("echo6 ip6_len = the frame's", "echo6 ip6_len one past the frame"),
                 ("echo4 ip_len = mtu", "echo4 ip_len = mtu + 1"),
                 ("echo6 ip6_len = mtu - 40", "echo6 ip6_len = mtu - 39"),
                 ("port6 flen 102", "port6 flen 101"), ("slot = reply", "slot = reply - 1"),
                 ("mac broadcast", "mac ff x 5"), ("mac 33 33", "mac 33 32"),
                 ("dst4 255.255.255.255", "dst4 255.255.255.255, no af-4 entry"),
                 ("port4 src ours", "port4 src foreign"), ("port6 src ours", "port6 src foreign"),
                 ("proto4 8 bytes", "proto4 7 bytes")):
        assert set(pair) <= names, pair


def test_census_every_action_in_the_grid_and_in_every_world(grid):
    assert {g[5] for g in grid} == set(model.ALL_ACTIONS)
    for name, (seed, n, slot) in cases.WORLDS.items():
        frames = cases.world(seed, n)
        acts = {a for a, _ in planned(frames, cases.socks_of(frames), cases.engine_table(), slot)}
        assert acts == set(model.ALL_ACTIONS), name


def all_replies(grid):
    """(request, action, reply, engine) of the grid and of one world."""
    out = [(fr, act, model.build(fr, act, eng, 0x1234), eng)
           for _, fr, _, eng, _, act, _ in grid if act in model.REPLIES]
    seed, n, slot = cases.WORLDS["slots"]
    frames, eng = cases.world(seed, n), cases.engine_table()
    for (fr, _), (act, _) in zip(frames, planned(frames, cases.socks_of(frames), eng, slot)):
        if act in model.REPLIES:
            out.append((fr, act, model.build(fr, act, eng, 7), eng))
    return out


def test_replies_are_not_udp_and_plan_to_none_at_the_other_end(grid):
    peer = cases.peer_table()
    seen = set()
    for fr, act, reply, _ in all_replies(grid):
        assert c_oracle.rx_verdict(reply, len(reply)) == NOT_UDP
        assert model.plan(reply, NOT_UDP, None, peer, 2048) == (model.NONE, 0)
        seen.add(act)
    assert seen == set(model.REPLIES)


def test_a_damaged_reply_is_a_bad_checksum_at_the_other_end(grid):
    # (the NONE above comes from a verified checksum, not from a filter)
    peer = cases.peer_table()
    for fr, act, reply, _ in all_replies(grid)[:40]:
        bad = cases.flip(reply, len(reply) - 1)
        assert model.plan(bad, NOT_UDP, None, peer, 2048) == (model.ICMP_BAD_CKSUM, 0)


def test_reply_fields(grid):
    for fr, act, reply, eng in all_replies(grid):
        v4 = act in (model.ECHO4, model.UNREACH_PORT4, model.UNREACH_PROTO4)
        assert reply[0:6] == fr[6:12] and reply[6:12] == bytes(eng[0]["mac"])
        if v4:
            assert reply[12:16] == b"\x08\x00\x45\x00" and reply[20:24] == b"\x40\x00\xff\x01"
            assert int.from_bytes(reply[16:18], "big") == len(reply) - 14
            assert reply[26:30] == cases.A4[0] and reply[30:34] == fr[26:30]
            assert c_oracle.ip_cksum(reply[14:34]) == 0
        else:
            assert reply[12:18] == b"\x86\xdd\x60\x00\x00\x00" and reply[20:22] == b"\x3a\xff"
            assert int.from_bytes(reply[18:20], "big") == len(reply) - 54
            assert reply[22:38] == cases.A6[0] and reply[38:54] == fr[22:38]


def test_checksums_are_the_references(grid):
    if not ref_oracle.available():
        pytest.skip("no oracle/_ref/libwc_ref.so and no reference tree (WC_REFERENCE_DIR) to "
                    "build it from")
    for fr, act, reply, _ in all_replies(grid):
        if reply[12:14] == b"\x08\x00":
            assert ref_oracle.ip_cksum(reply[34:]) == 0
            assert ref_oracle.ip_cksum(reply[14:34]) == 0
        else:
            assert ref_oracle.payload_cksum(reply[14:], len(reply) - 14) == 0
    # the plan's two checksum decisions on the request side
    seed, n, _ = cases.WORLDS["packed"]
    reqs = [(g[1], g[3]) for g in grid] + [(fr, cases.engine_table()) for fr, _ in cases.world(seed, n)]
    n4 = n6 = 0
    for fr, eng in reqs:
        if c_oracle.rx_verdict(fr, len(fr)) != NOT_UDP:
            continue
        act, _ = model.plan(fr, NOT_UDP, None, eng, 65535)
        if act == model.FILTERED:
            continue
        if fr[12:14] == b"\x08\x00" and fr[23] == 1:
            hl = (fr[14] & 15) * 4
            ln = min((int.from_bytes(fr[16:18], "big") - hl) & 0xFFFF, len(fr) - 14 - hl)
            bad = ref_oracle.ip_cksum(fr[14 + hl:14 + hl + ln]) != 0
            n4 += 1
        elif fr[12:14] == b"\x86\xdd" and fr[20] == 58:
            ln = min(int.from_bytes(fr[18:20], "big"), len(fr) - 54)
            bad = ref_oracle.payload_cksum(fr[14:54 + ln], 40 + ln) != 0
            n6 += 1
        else:
            continue
        assert (act == model.ICMP_BAD_CKSUM) == bad
    assert n4 > 20 and n6 > 20
