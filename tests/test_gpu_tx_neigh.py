"""GPU tests of the TX neighbours (wc_neigh_tab_init, wc_neigh_apply,
wc_tx_resolve, wc_tx_hold_plan, wc_tx_solicit_build) against
tests/tx_neigh_model.py, all exact: the cache read back through wc_tx_resolve
and through a D2H copy with wc_neigh_tab_lookup / wc_neigh_tab_stats, the whole
destination table byte for byte, lists and counts, the whole output buffer
(random fill, gaps and guard bytes included), and the closed loop -- resolve,
solicit, the peers' answers through the real RX calls, apply, resolve, hold
plan, TX build, RX verdict -- on the device end to end."""
import numpy as np
import pytest
import torch

import rx_reply_cases as rc
import tx_neigh_cases as cases
import tx_neigh_model as model
import warpcore_amd as wc

pytestmark = pytest.mark.gpu


def dev_bytes(a: np.ndarray, dev):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)


def dev_count(n: int, dev):
    return torch.tensor([n], dtype=torch.int64, device=dev)


def apply(tab, upd: np.ndarray, count: int, m: int = None, dropped=None):
    """neigh_apply of an UPDATE array with *d_count = count; the dropped count."""
    d = tab.device
    m = upd.size if m is None else m
    out = wc.neigh_apply(tab, dev_bytes(upd, d).reshape(-1, 24), dev_count(count, d), m, dropped)
    return int(out.item())


def host_view(tab):
    torch.cuda.synchronize()
    return tab.cpu().numpy()


def lookups(tab, ks):
    h = host_view(tab)
    return [wc.neigh_tab_lookup(h, af, a) for af, a in ks]


def resolved(tab, ks):
    """The same lookups through wc_tx_resolve: None for a miss."""
    dsts = cases.dst_table([(a, 9) for _, a in ks])
    afs = np.array([af for af, _ in ks], np.uint8)
    d_dsts = dev_bytes(dsts, tab.device)
    state, _, _ = wc.tx_resolve(tab, d_dsts, torch.from_numpy(afs).to(tab.device), want_list=False)
    after = d_dsts.cpu().numpy().view(model.DST)
    return [bytes(after["dmac"][k]) if s == wc.NR_READY else None
            for k, s in enumerate(state.cpu().numpy())]


def want_lookups(cache, ks):
    return [cache.get(model.key(af, a)) for af, a in ks]


def check_table(tab, cache, ks, cap):
    want = want_lookups(cache, ks)
    assert lookups(tab, ks) == want
    assert resolved(tab, ks) == [None if m == model.BCAST else m for m in want]
    assert wc.neigh_tab_stats(host_view(tab)) == (cap, len(cache))


@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_apply_batches_and_every_m(gpu, n):
    """cap 64: repeats, look-alikes, af 0 and af 7 records, m below and above
    the count, three applies in a row on one table, two fresh tables alike."""
    recs, ks = cases.record_world(100 + n, 3 * n, 20)
    probe = ks + [(4, cases.addr4(9999)), (6, cases.addr6(9999))]
    tabs = [wc.neigh_tab_init(64, gpu), wc.neigh_tab_init(64, gpu)]
    cache = {}
    for r, (count, m) in enumerate(((n, n), (n - 1, n), (n + 5, n))):
        upd = model.records(recs[r * n:(r + 1) * n])
        want = model.apply(cache, upd, count, m)
        for tab in tabs:
            assert apply(tab, upd, count, m) == want
            check_table(tab, cache, probe, 64)
    assert lookups(tabs[0], probe) == lookups(tabs[1], probe)
    if n >= 63:
        assert len(cache) == len(ks) and want > 0
    # a second init is the flush
    wc.neigh_tab_init(64, tab=tabs[0])
    check_table(tabs[0], {}, probe, 64)


def test_the_same_key_inside_one_wave_and_across_workgroups(gpu):
    recs = cases.same_key_burst(700)
    upd = model.records(recs)
    cache = {}
    model.apply(cache, upd, len(recs), len(recs))
    ks = [(6, cases.addr6(1)), (4, cases.addr4(2))] + cases.lookalikes()
    dropped = torch.zeros(1, dtype=torch.int64, device=gpu)
    for _ in range(2):
        tab = wc.neigh_tab_init(64, gpu)
        assert apply(tab, upd, len(recs), dropped=dropped) == 0
        check_table(tab, cache, ks, 64)
    assert cache[(4, cases.addr4(2))] == recs[-2][1] and cache[(6, cases.addr6(1))] == recs[-1][1]
    # the look-alikes are two keys, and an accumulated counter keeps counting
    la = cases.lookalikes()
    upd = model.records([(la[0][0], b"\x02" * 6, la[0][1]), (la[1][0], b"\x03" * 6, la[1][1]),
                         (7, b"\x04" * 6, la[0][1]), (9, b"\x04" * 6, la[0][1])])
    model.apply(cache, upd, 4, 4)
    assert apply(tab, upd, 4, dropped=dropped) == 2
    check_table(tab, cache, ks, 64)
    assert lookups(tab, la) == [b"\x02" * 6, b"\x03" * 6]


def test_wrapping_probes(gpu):
    ks = cases.wrap_keys(64, 40)
    rng = np.random.default_rng(8)
    recs = [(af, cases.mac_of(rng), a) for af, a in ks] * 2
    upd = model.records(recs)
    cache = {}
    model.apply(cache, upd, len(recs), len(recs))
    tab = wc.neigh_tab_init(64, gpu)
    assert apply(tab, upd, len(recs)) == 0
    check_table(tab, cache, ks + cases.lookalikes(), 64)


def test_full_table_rule(gpu):
    """80 distinct keys, three records each, into cap 64: used == 64, every
    present key has its last MAC, dropped = the records of absent keys -- not a
    particular survivor set (which of the new keys a full table keeps is
    unspecified, and two runs may keep different ones: seen on the device); a
    further apply overwrites and still cannot insert."""
    ks = cases.keys(80)
    rng = np.random.default_rng(6)
    recs = [(af, cases.mac_of(rng), a) for _ in range(3) for af, a in ks]
    recs = [recs[i] for i in rng.permutation(len(recs))]
    upd = model.records(recs)
    last = {}
    model.apply(last, upd, len(recs), len(recs))
    looks = []
    for _ in range(2):
        tab = wc.neigh_tab_init(64, gpu)
        dropped = apply(tab, upd, len(recs))
        look = lookups(tab, ks)
        present = [k for k, mac in zip(ks, look) if mac is not None]
        assert len(present) == 64 and wc.neigh_tab_stats(host_view(tab)) == (64, 64)
        assert dropped == 3 * (80 - 64)
        for (af, a), mac in zip(ks, look):
            assert mac is None or mac == last[model.key(af, a)]
        assert resolved(tab, ks) == look
        looks.append(look)
    again = model.records([(af, cases.mac_of(rng), a) for af, a in ks])
    assert apply(tab, again, 80) == 80 - 64
    for (af, a), old, new, rec in zip(ks, looks[1], lookups(tab, ks), again):
        assert (old is None) == (new is None) and (new is None or new == bytes(rec["mac"]))


@pytest.mark.parametrize("ndst", [0, 1, 63, 64, 65, 257, 4097])
def test_resolve(gpu, ndst):
    recs, ks = cases.record_world(21, 200, 30)
    bc = (4, cases.addr4(77) + bytes(12))  # a cached broadcast MAC is unresolved
    recs.append((4, model.BCAST, bc[1]))
    upd = model.records(recs)
    cache = {}
    model.apply(cache, upd, len(recs), len(recs))
    tab = wc.neigh_tab_init(256, gpu)
    apply(tab, upd, len(recs))
    dsts, afs = cases.dst_world(ndst, ndst, ks + [bc])
    if ndst >= 257:  # duplicates far apart, beside the adjacent ones of dst_world
        dsts["addr"][ndst - 1], afs[ndst - 1] = dsts["addr"][1], afs[1]
        far = (4, cases.addr4(60000) + bytes(12))
        for k in (3, ndst - 3):
            dsts["addr"][k], afs[k] = np.frombuffer(far[1], np.uint8), 4
    state, after, lst = model.resolve(cache, dsts, afs)
    d_dsts, d_af = dev_bytes(dsts, gpu), torch.from_numpy(afs).to(gpu)
    got = []
    for _ in range(2):  # the same input again gives the same output
        d_dsts = dev_bytes(dsts, gpu)
        g_state, g_list, g_count = wc.tx_resolve(tab, d_dsts, d_af)
        cnt = int(g_count.item())
        got.append((g_state.cpu().numpy(), d_dsts.cpu().numpy(),
                    g_list.cpu().numpy().view(np.uint32)[:cnt]))
    for g_state, g_dsts, g_list in got:
        bad = np.flatnonzero(g_state != state)
        assert bad.size == 0, (bad[:8], g_state[bad[:8]], state[bad[:8]])
        assert g_dsts.tobytes() == after.tobytes()  # addr and port unchanged, BAD_AF untouched
        assert g_list.tolist() == lst.tolist() and (np.diff(g_list.astype(np.int64)) > 0).all()
    if ndst >= 63:
        assert {int(x) for x in state} == {wc.NR_READY, wc.NR_BAD_AF, wc.NR_MISS, wc.NR_MISS_DUP}
    if ndst >= 257:
        assert state[3] == wc.NR_MISS and state[ndst - 3] == wc.NR_MISS_DUP
        assert any(bytes(after["dmac"][k]) == model.BCAST and cache.get(
            model.key(int(afs[k]), bytes(dsts["addr"][k]))) == model.BCAST for k in range(ndst))
    # without a list
    d_dsts = dev_bytes(dsts, gpu)
    g_state, none_list, none_count = wc.tx_resolve(tab, d_dsts, d_af, want_list=False)
    assert none_list is None and none_count is None and (g_state.cpu().numpy() == state).all()


@pytest.mark.parametrize("n", [1, 64, 65, 1000])
def test_hold_plan(gpu, n):
    g = cases.hold_grid()
    socks = cases.socks_table()
    afs = np.array([a for a, _ in cases.HOLD_DSTS], np.uint8)
    state = np.array([s for _, s in cases.HOLD_DSTS], np.uint8)
    descs = cases.descs_of([(s, t) for _, s, t, _ in g]) if n == 64 else cases.hold_world(n, n)
    if n == 64:
        descs = np.concatenate([descs] * 5)[:64]
    want, lst = model.hold(descs, socks, state, afs)
    hold, g_list, g_count = wc.tx_hold_plan(dev_bytes(descs, gpu), dev_bytes(socks, gpu),
                                            torch.from_numpy(state).to(gpu),
                                            torch.from_numpy(afs).to(gpu))
    cnt = int(g_count.item())
    assert (hold.cpu().numpy() == want).all()
    assert cnt == len(lst) and g_list.cpu().numpy().view(np.uint32)[:cnt].tolist() == lst.tolist()
    if n >= 64:
        assert set(want.tolist()) == {wc.TH_READY, wc.TH_MALFORMED, wc.TH_HELD}
    if n == 64:
        for (name, _, _, code), h in zip(g, hold.cpu().numpy()):
            assert h == code, name
    # no destination table: unconnected frames are malformed; no list asked
    want, _ = model.hold(descs, socks, None, None)
    hold, a, b = wc.tx_hold_plan(dev_bytes(descs, gpu), dev_bytes(socks, gpu), None, None,
                                 want_list=False)
    assert a is None and b is None and (hold.cpu().numpy() == want).all()


def solicit(gpu, dsts, afs, lst, count, eng, slot, m, seed=0):
    rng = np.random.default_rng(3000 + seed)
    out0, offs = rc.out_slots(m, slot, rng)
    d_out = torch.from_numpy(out0.copy()).to(gpu)
    padded = np.zeros(max(m, len(lst), 1), np.uint32)  # (a list holds min(m, ndst) entries at least)
    padded[:len(lst)] = lst
    d_list = torch.from_numpy(padded.view(np.int32).copy()).to(gpu)
    olen, built = wc.tx_solicit_build(dev_bytes(dsts, gpu), torch.from_numpy(afs).to(gpu), d_list,
                                      dev_count(count, gpu), dev_bytes(eng, gpu), d_out,
                                      torch.from_numpy(offs).to(gpu), slot)
    torch.cuda.synchronize()
    want_out, want_len, want_built = model.built(out0, offs, slot, dsts, afs, lst, count, eng)
    got = d_out.cpu().numpy()
    assert (olen.cpu().numpy() == want_len).all() and int(built.item()) == want_built
    diff = np.flatnonzero(got != want_out)
    assert diff.size == 0, f"{diff.size} output bytes differ, the first at {diff[:4]}"
    return got, offs, want_len, want_built


@pytest.mark.parametrize("slot", [41, 42, 85, 86, 87, 2048])
def test_solicit_build_slots_at_every_phase(gpu, slot):
    dsts, afs = cases.dst_world(slot, 300, cases.keys(10), hit=0.2)
    lst = np.flatnonzero((afs == 4) | (afs == 6)).astype(np.uint32)[:200]
    lst = np.concatenate([lst, np.array([300, 307, 0xFFFFFFFF], np.uint32),  # stale indices
                          np.flatnonzero((afs != 4) & (afs != 6)).astype(np.uint32)[:5]])
    np.random.default_rng(slot).shuffle(lst)
    eng = rc.engine_table(rng=np.random.default_rng(slot))
    for count, m in ((len(lst), len(lst)), (len(lst), len(lst) - 9), (len(lst) - 9, len(lst) + 4),
                     (0, 3)):
        _, offs, lens, built = solicit(gpu, dsts, afs, lst, count, eng, slot, m, seed=m)
        seen = set(lens.tolist())
        if count and slot >= 86:
            assert seen == {0, 42, 86} and built == min(count, m) - sum(
                1 for i in lst[:min(count, m)] if i >= 300 or afs[i] not in (4, 6))
            assert {int(o) % 16 for o, ln in zip(offs, lens) if ln == 86} == set(range(16))
            assert {int(o) % 16 for o, ln in zip(offs, lens) if ln == 42} == set(range(16))
        elif count:
            assert seen == ({0, 42} if slot >= 42 else {0})
        else:
            assert seen == {0} and built == 0


def test_solicit_build_known_answers_and_engines_without_a_family(gpu):
    dsts = cases.dst_table([(cases.PEER4, 1), (cases.PEER6, 2)])
    afs = np.array([4, 6], np.uint8)
    lst = np.array([0, 1], np.uint32)
    out, offs, lens, built = solicit(gpu, dsts, afs, lst, 2, rc.engine_table(), 86, 2)
    got = [out[int(o):int(o) + int(ln)].tobytes().hex() for o, ln in zip(offs, lens)]
    assert got == [cases.ARP_WHO_HAS_HEX, cases.NSOL_HEX] and built == 2
    for eng, want in ((rc.engine_table(v4=0), [0, 86]), (rc.engine_table(v6=0), [42, 0]),
                      (rc.engine_table(v4=0, v6=0), [0, 0])):
        _, _, lens, built = solicit(gpu, dsts, afs, lst, 2, eng, 2048, 2)
        assert lens.tolist() == want and built == sum(x != 0 for x in want)
    # ndst = 0: zero lengths, nothing written
    empty = np.zeros(0, model.DST)
    _, _, lens, built = solicit(gpu, empty, np.zeros(0, np.uint8), lst, 2, rc.engine_table(), 86, 2)
    assert not lens.any() and built == 0


def rx_chain(d_buf, d_off, d_len, d_eng):
    """rx_verdict_ragged -> rx_reply_plan -> rx_neigh_plan over one ring."""
    v, _ = wc.rx_verdict_ragged(d_buf, d_off, d_len)
    act, _, _, _ = wc.rx_reply_plan(d_buf, d_off, d_len, v, None, d_eng, 2048, want_list=False)
    nact, rl, rcnt, ul, ucnt = wc.rx_neigh_plan(d_buf, d_off, d_len, act, d_eng)
    return act, nact, rl, rcnt, ul, ucnt


def test_closed_loop_on_the_device(gpu):
    """A dozen peers, both families: nothing between the first resolve and the
    built frames' Ethernet destinations is worked out on the host."""
    peers = cases.peers(12)
    eng = rc.engine_table()
    d_eng = dev_bytes(eng, gpu)
    dsts = cases.dst_table([(a4, 4433) for _, a4, _ in peers] + [(a6, 4433) for _, _, a6 in peers] +
                           [(peers[0][1], 4434), (peers[5][2], 4434)], np.random.default_rng(1))
    afs = np.array([4] * 12 + [6] * 12 + [4, 6], np.uint8)
    ndst = len(afs)
    d_dsts, d_af = dev_bytes(dsts, gpu), torch.from_numpy(afs).to(gpu)
    tab = wc.neigh_tab_init(64, gpu)

    # 1. resolve: every address misses, the two repeats are duplicates
    state, miss_list, miss_count = wc.tx_resolve(tab, d_dsts, d_af)
    assert state.cpu().tolist() == [wc.NR_MISS] * 24 + [wc.NR_MISS_DUP] * 2
    assert int(miss_count.item()) == 24
    # 2. solicit build
    rng = np.random.default_rng(2)
    ring0, ring_off = rc.out_slots(ndst, 128, rng)
    d_ring, d_ring_off = torch.from_numpy(ring0.copy()).to(gpu), torch.from_numpy(ring_off).to(gpu)
    sol_len, sol_built = wc.tx_solicit_build(d_dsts, d_af, miss_list, miss_count, d_eng, d_ring,
                                             d_ring_off, 128)
    assert int(sol_built.item()) == 24
    want_ring, want_len, _ = model.built(ring0, ring_off, 128, dsts, afs, np.arange(24), 24, eng)
    assert (d_ring.cpu().numpy() == want_ring).all() and (sol_len.cpu().numpy() == want_len).all()
    # 3. the solicitations as an RX ring under each peer's own table: each peer
    #    answers the two that ask for it
    reply0, reply_off = rc.out_slots(24, 128, rng)
    d_reply = torch.from_numpy(reply0.copy()).to(gpu)
    reply_len = torch.zeros(24, dtype=torch.uint16, device=gpu)
    findings = []
    for p, (mac, a4, a6) in enumerate(peers):
        d_peer = dev_bytes(cases.peer_engine(mac, a4, a6), gpu)
        act, nact, rl, rcnt, _, _ = rx_chain(d_ring, d_ring_off, sol_len, d_peer)
        codes = nact.cpu().numpy()
        # the models' prediction: the who-has for another host updates the peer's
        # cache (arp.c:181-183, 196), the solicitation for another is filtered
        want = np.zeros(ndst, np.uint8)
        want[:12] = wc.RN_UPDATE4
        want[p], want[12 + p] = wc.RN_ARP_IS_AT, wc.RN_NADV
        if not (codes == want).all():
            findings.append((p, codes.tolist()))
        off = torch.from_numpy(reply_off[2 * p:2 * p + 2]).to(gpu)
        olen, built = wc.rx_neigh_build(d_ring, d_ring_off, sol_len, nact, rl, rcnt, d_peer, d_reply,
                                        off, 128)
        assert int(built.item()) == 2
        reply_len.view(torch.int16)[2 * p:2 * p + 2] = olen.view(torch.int16)
    assert not findings, findings  # the existing calls treat a solicitation as the models predict
    # 4. the replies as an RX ring under our table, through the same calls and the update records
    d_reply_off = torch.from_numpy(reply_off).to(gpu)
    act, nact, _, _, ul, ucnt = rx_chain(d_reply, d_reply_off, reply_len, d_eng)
    assert (act.cpu().numpy() == wc.RR_HOST).all() and int(ucnt.item()) == 24
    assert set(nact.cpu().tolist()) == {wc.RN_UPDATE4, wc.RN_UPDATE6}
    upd = wc.rx_neigh_updates(d_reply, d_reply_off, reply_len, nact, ul, ucnt, 32)
    # 5. apply
    dropped = wc.neigh_apply(tab, upd, ucnt)
    assert int(dropped.item()) == 0
    # 6. resolve again: all READY, with the peers' MACs
    state, miss_list, miss_count = wc.tx_resolve(tab, d_dsts, d_af)
    assert not state.cpu().numpy().any() and int(miss_count.item()) == 0
    after = d_dsts.cpu().numpy().view(model.DST)
    macs = [p[0] for p in peers]
    assert [bytes(m) for m in after["dmac"]] == macs + macs + [macs[0], macs[5]]
    assert (after["addr"] == dsts["addr"]).all() and (after["port"] == dsts["port"]).all()
    assert wc.neigh_tab_stats(host_view(tab)) == (64, 24)
    # 7. hold plan: none held
    socks = cases.socks_table()[:2]
    socks["lport"] = 0x5111  # port 4433 as stored
    descs = cases.descs_of([(0 if afs[t] == 4 else 1, t) for t in range(ndst)] * 3)
    d_descs, d_socks = dev_bytes(descs, gpu), dev_bytes(socks, gpu)
    hold, held, held_count = wc.tx_hold_plan(d_descs, d_socks, state, d_af)
    assert not hold.cpu().numpy().any() and int(held_count.item()) == 0
    # 8. TX build, 9. the frames' Ethernet destinations and the RX verdict
    n = len(descs)
    tx_off = np.arange(n, dtype=np.uint64) * 256 + 3
    d_tx = torch.from_numpy(rng.integers(0, 256, n * 256 + 64, dtype=np.uint8)).to(gpu)
    d_tx_off = torch.from_numpy(tx_off).to(gpu)
    flen, status, _, _, errors = wc.tx_build_ragged(d_tx, d_tx_off, d_descs, d_socks, d_dsts, 256)
    assert int(errors.item()) == 0 and (status.cpu().numpy() == wc.TX_SEALED).all()
    verdict, _ = wc.rx_verdict_ragged(d_tx, d_tx_off, flen)
    assert (verdict.cpu().numpy() == wc.RX_OK).all()
    tx = d_tx.cpu().numpy()
    for i in range(n):
        o = int(tx_off[i])
        assert tx[o:o + 6].tobytes() == bytes(after["dmac"][int(descs["dst"][i])])
        assert tx[o + 6:o + 12].tobytes() == rc.MAC
