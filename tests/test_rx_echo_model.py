"""CPU tests of the RX echo's model (tests/rx_echo_model.py) on the worlds of
tests/rx_echo_cases.py: the echo order against a per-socket walk written the
way inetd.c reads, and the swap properties of every ECHO entry -- its
descriptor, destination and payload taken through tx_build_model give a frame
that rx_deliver_model accepts as the request's answer -- and the inert entries
refused by the build."""
import numpy as np
import pytest

import rx_deliver_model as dmodel
import rx_echo_cases as cases
import rx_echo_model as model
import tx_build_model as bmodel
from rx_reply_cases import out_slots, packed

SLOT = 2048


@pytest.fixture(scope="module")
def ring():
    socks, frames = cases.world(31, 300, 17)
    buf, offs, lens = packed([(fr, None) for fr in frames], np.random.default_rng(5), 3)
    return socks, buf, offs, lens, cases.plan(buf, offs, lens, socks)


def inetd_walk(p, emap):
    """inetd.c:161-169, one socket after another: sl_foreach over the sockets,
    w_rx takes the socket's queue in arrival order, port 7 hands all of it to
    w_tx; a socket that is off discards.  -> [(socket, frame index)]"""
    out = []
    for s in range(len(emap)):
        if int(emap[s]) > 255:
            continue
        queue = [i for i in range(len(p.sock)) if int(p.sock[i]) == s]  # sq_insert_tail order
        out += [(s, i) for i in queue]
    return out


@pytest.mark.parametrize("kind", ["all", "none", "alternating", "single"])
def test_order_is_the_per_socket_walk(ring, kind):
    socks, buf, offs, lens, p = ring
    emap = cases.echo_map(len(socks), kind, one=5)
    want = inetd_walk(p, emap)
    for copy in (True, False):
        for m in (0, max(len(want) - 1, 0), len(want), len(want) + 5):
            e = model.echo(buf, offs, lens, p.rec, p.list, p.start, emap, m, copy, SLOT)
            assert e.E == len(want)
            k = min(m, e.E)
            assert [(e.sock[j], int(e.src[j])) for j in range(k)] == want[:k]
            assert (e.status[:k] == model.ECHO).all() and (e.status[k:] == model.NONE).all()
            assert (e.src[k:] == model.NO_FRAME).all() and e.skipped == 0
    if kind == "all":
        assert len(want) == int(p.start[254]) > 150, "every frame a socket took is echoed"


def test_the_world_holds_what_it_promises(ring):
    socks, buf, offs, lens, p = ring
    took = np.flatnonzero(p.sock < len(socks))
    rec = p.rec[took]
    assert set(cases.LENS) <= set(rec["data_len"].tolist())
    assert {4, 6} <= set(rec["af"].tolist())
    assert set(range(20, 64, 4)) <= set(rec["hl"][rec["af"] == 4].tolist()), "IHL 5 to 15"
    assert (p.verdicts[took] == dmodel.OK_NO_CKSUM).any(), "zero UDP checksums"
    assert {0, 1} <= set(socks["connected"][np.unique(p.sock[took])].tolist())
    assert (p.sock == 0xFF).any() and (p.sock == 0xFE).any(), "strays and frames that are not UDP"


def swapped(request: bytes, rq, built: bytes):
    """The built frame is the request's answer: accepted, the same payload, the
    ports and the addresses swapped.  The TOS is the request's, except that
    mk_ip6_hdr keeps a traffic class only with ECN bits in it (ip6.c:133, the
    TX build's contract): an IPv6 request with (tos & 3) == 0 is answered with
    TOS 0 by the reference too."""
    ra = dmodel.record_of(built, len(built))
    af = int(rq["af"])
    assert int(ra["af"]) == af, "rx_deliver_model accepts the built frame"
    n = 4 if af == 4 else 16
    pay = lambda f, r: f[int(r["data_off"]):int(r["data_off"]) + int(r["data_len"])]  # noqa: E731
    assert pay(built, ra) == pay(request, rq)
    tos = int(rq["tos"])
    assert int(ra["tos"]) == (tos if af == 4 or tos & 3 else 0)
    assert (int(ra["sport"]), int(ra["dport"])) == (int(rq["dport"]), int(rq["sport"]))
    at = lambda f, o: f[o:o + n]  # noqa: E731
    assert at(built, int(ra["src_off"])) == at(request, int(rq["dst_off"]))
    assert at(built, int(ra["dst_off"])) == at(request, int(rq["src_off"]))
    assert built[:6] == request[6:12], "without a pump the placeholder is the Ethernet destination"


@pytest.mark.parametrize("copy", [True, False], ids=["copy", "in_place"])
def test_every_echo_entry_builds_the_answer(ring, copy):
    socks, buf, offs, lens, p = ring
    emap = cases.echo_map(len(socks), "all")
    E = model.echo(buf, offs, lens, p.rec, p.list, p.start, emap, 0, copy, SLOT).E
    m = E + 5
    ids = np.random.default_rng(2).integers(0, 1 << 16, m).astype(np.uint16)
    e = model.echo(buf, offs, lens, p.rec, p.list, p.start, emap, m, copy, SLOT, ip_ids=ids)
    tx = cases.tx_socks(socks)
    if copy:
        tbuf, toff = out_slots(m, SLOT, np.random.default_rng(3))
        for j in range(m):
            if e.payload[j] is not None:
                at = int(toff[j]) + bmodel.hdr_len(int(e.af[j]))
                tbuf[at:at + len(e.payload[j])] = np.frombuffer(e.payload[j], np.uint8)
        slot = SLOT
    else:
        tbuf, toff, slot = buf.copy(), e.tx_off, SLOT - 40
    before = tbuf.copy()
    b = bmodel.Expect(tbuf, toff, e.desc, tx, e.dsts, slot)
    assert (b.status[:E] == bmodel.SEALED).all() and (e.status[:E] == model.ECHO).all()
    for j in range(E):
        i = int(e.src[j])
        o, flen = int(toff[j]), int(b.frame_len[j])
        request = buf[int(offs[i]):int(offs[i]) + int(lens[i])].tobytes()
        swapped(request, p.rec[i], b.buf[o:o + flen].tobytes())
        if not copy:  # the built frame ends where the request's payload ends
            assert o == int(offs[i]) + int(p.rec[i]["hl"]) - model.hl_tx(int(e.af[j]))
            assert o + flen == int(offs[i]) + int(p.rec[i]["data_off"]) + int(p.rec[i]["data_len"])
    # the inert entries: refused, nothing written
    assert (b.status[E:] == bmodel.MALFORMED).all() and (b.frame_len[E:] == 0).all()
    assert b.errors == m - E
    touched = np.zeros(len(tbuf), bool)
    for j in range(E):
        touched[int(toff[j]):int(toff[j]) + bmodel.hdr_len(int(e.af[j]))] = True
    assert (b.buf[~touched] == before[~touched]).all()


def test_forged_records_and_small_slots(ring):
    socks, buf, offs, lens, p = ring
    emap = cases.echo_map(len(socks), "all")
    base = model.echo(buf, offs, lens, p.rec, p.list, p.start, emap, 400, True, SLOT)
    E = base.E
    rec, lst = p.rec.copy(), p.list.copy()
    i0, i1, i2 = (int(base.src[j]) for j in (0, 1, 2))
    rec[i0]["data_len"] = int(lens[i0]) - int(rec[i0]["data_off"]) + 1   # one byte past the frame
    rec[i1]["data_len"] = int(lens[i1]) - int(rec[i1]["data_off"])       # the exact fit
    rec[i2]["af"] = 5
    lst[int(p.start[0]) + 3] = len(offs)                                 # names no frame
    # records no delivery writes, one rule of STALE each
    i4, i5, i6 = (int(base.src[j]) for j in (4, 5, 6))
    rec[i4]["hl"], rec[i4]["data_off"] = 16, 14 + 16 + 8                 # below the built header
    rec[i5]["data_off"] = int(rec[i5]["data_off"]) - 1                   # not 14 + hl + 8
    rec[i6]["src_off"] = int(lens[i6]) - (4 if int(rec[i6]["af"]) == 4 else 16) + 1
    e = model.echo(buf, offs, lens, rec, lst, p.start, emap, 400, True, SLOT)
    assert e.E == E
    assert e.status[:7].tolist() == [model.SHORT, model.ECHO] + [model.STALE] * 5
    assert e.skipped == 6 and e.src[3] == model.NO_FRAME and e.src[0] == i0
    for k, only in ((i4, "hl"), (i5, "data_off"), (i6, "src_off")):   # each by its own rule alone
        r = rec[k].copy()
        r[only] = p.rec[k][only]
        if only == "hl":
            r["data_off"] = p.rec[k]["data_off"]
        assert model.status_of(k, len(offs), r, int(lens[k]), True, SLOT) == model.ECHO
    for j in (0, 2, 3, 4, 5, 6):
        assert e.payload[j] is None and e.af[j] == 0 and not e.dsts[j].tobytes().strip(b"\0")
        assert e.desc[j].tolist() == (0xFFFF, 0, 0, 0, j)
    # the slot bound at the exact fit and one below it
    j = int(np.flatnonzero(base.desc["data_len"][:E] == 200)[0])
    fit = bmodel.hdr_len(int(base.af[j])) + 200
    for slot, want in ((fit, model.ECHO), (fit - 1, model.NO_ROOM)):
        for copy in (True, False):
            e = model.echo(buf, offs, lens, p.rec, p.list, p.start, emap, 400, copy, slot)
            assert e.status[j] == (want if copy else model.ECHO)
    # stale starts: a decreasing pair and one above n empty their runs alone
    start = p.start.copy()
    start[3] = start[2] - 1 if start[2] else start[3]
    e = model.echo(buf, offs, lens, p.rec, p.list, start, emap, 400, True, SLOT)
    lens_of = model.run_lengths(start, emap, len(offs))
    assert e.E == sum(lens_of) and lens_of[2] == 0
    start = p.start.copy()
    start[len(socks)] = len(offs) + 1
    assert model.run_lengths(start, emap, len(offs))[len(socks) - 1] == 0
