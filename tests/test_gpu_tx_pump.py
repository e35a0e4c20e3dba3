"""GPU tests of the TX pump (wc_tx_pump): all thirteen outputs, the destination
table, the frame buffer and the solicitation buffer against tests/tx_pump_model
-- the models alone -- AND against the chain run on copies of the same tensors
(tx_resolve -> tx_hold_plan -> tx_solicit_build, then tx_build_ragged on the
READY subset, which the test gathers on the host from the chain's own hold bytes
and scatters back), bit-exact.  Every output array is pre-filled with 0xA5 and
stands between guard bytes; the two buffers are compared whole, so untouched
frames, payload bytes, gaps and guards keep their bytes; list entries at and
past a count keep theirs; *errors starts at 7 and is added to."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import rx_drain_cases as dcases
import rx_reply_cases as rc
import tx_build_model as bmodel
import tx_neigh_cases as nc
import tx_neigh_model as nmodel
import tx_pump_cases as cases
import tx_pump_model as model
import warpcore_amd as wc
from warpcore_amd import _lib
from warpcore_amd.cksum import _PumpOut

pytestmark = pytest.mark.gpu

FILL, GUARD, ERRORS0 = 0xA5, 64, 7
SMALL, SMALL_DST = cases.SMALL, cases.SMALL_DST
assert (SMALL, SMALL_DST, model.PUMP_HELD) == (wc.TX_PUMP_SMALL, wc.TX_PUMP_SMALL_DST, wc.TX_PUMP_HELD)
LISTS = {"miss_list": "miss_count", "held_list": "held_count"}


def dev(a: np.ndarray, d) -> torch.Tensor:
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to(d)


def dev_bytes(a: np.ndarray, d) -> torch.Tensor:
    return dev(np.ascontiguousarray(a).view(np.uint8).reshape(-1), d)


class Outs:
    """wc_tx_pump's thirteen arrays, each 0xA5-filled between 64 guard bytes."""

    def __init__(self, d, n: int, ndst: int, m: int, errors: int = ERRORS0):
        spec = {"state": (ndst, torch.uint8), "miss_list": (4 * max(ndst, 1), torch.int32),
                "miss_count": (8, torch.int64), "hold": (n, torch.uint8),
                "held_list": (4 * max(n, 1), torch.int32), "held_count": (8, torch.int64),
                "sol_lens": (2 * m, torch.uint16), "sol_built": (8, torch.int64),
                "frame_lens": (2 * n, torch.uint16), "status": (n, torch.uint8),
                "ip_hdr": (2 * n, torch.uint16), "udp": (2 * n, torch.uint16),
                "errors": (8, torch.int64)}
        assert list(spec) == list(wc.TxPump._fields)
        self.raw, self.nbytes, views = {}, {}, {}
        for name, (nbytes, dtype) in spec.items():
            raw = torch.full((2 * GUARD + nbytes,), FILL, dtype=torch.uint8, device=d)
            self.raw[name], self.nbytes[name] = raw, nbytes
            views[name] = raw[GUARD:GUARD + nbytes].view(dtype)
        views["errors"].fill_(errors)
        self.out = wc.TxPump(**views)

    def fetch(self):
        """Everything to the host; the guards checked."""
        self.host = {k: r.cpu().numpy() for k, r in self.raw.items()}
        for name, h in self.host.items():
            nb = self.nbytes[name]
            assert (h[:GUARD] == FILL).all() and (h[GUARD + nb:] == FILL).all(), f"guard of {name}"
        return self

    def get(self, name: str, dtype=np.uint8) -> np.ndarray:
        return self.host[name][GUARD:GUARD + self.nbytes[name]].view(dtype)

    def count(self, name: str) -> int:
        return int(self.get(name, np.uint64)[0])


def make_tab(d, cache: dict, cap: int = None) -> torch.Tensor:
    cap = cap or max(64, 1 << (4 * max(len(cache), 1)).bit_length())
    tab = wc.neigh_tab_init(cap, d)
    if cache:
        upd = cases.records_of(cache)
        dropped = wc.neigh_apply(tab, dev_bytes(upd, d).reshape(-1, 24),
                                 torch.tensor([upd.size], dtype=torch.int64, device=d))
        assert int(dropped.item()) == 0
    return tab


class Dev:
    """A world's read-only inputs on the device; fresh(): the three tensors a
    call writes into (destination table, frames, solicitation slots)."""

    def __init__(self, d, w, tab=None):
        self.d, self.w = d, w
        self.tab = make_tab(d, w.cache) if tab is None else tab
        self.af = dev(w.afs, d) if w.ndst else None
        self.descs, self.socks = dev_bytes(w.descs, d), dev_bytes(w.socks, d)
        self.offs, self.eng = dev(w.offs, d), dev_bytes(w.eng, d)
        self.sol_offs = dev(w.sol_offs, d)

    def fresh(self):
        w, d = self.w, self.d
        return SimpleNamespace(dsts=dev_bytes(w.dsts, d) if w.ndst else None, buf=dev(w.buf, d),
                               sol=dev(w.sol, d))

    def run(self, zero_udp=False, outs=None, mem=None, scratch=None, stream=None):
        w = self.w
        outs = Outs(self.d, w.n, w.ndst, w.m) if outs is None else outs
        mem = self.fresh() if mem is None else mem
        wc.tx_pump(self.tab, mem.dsts, self.af, self.descs, self.socks, mem.buf, self.offs, w.slot,
                   self.eng, mem.sol, self.sol_offs, cases.SOL_SLOT, zero_udp=zero_udp, out=outs.out,
                   scratch=scratch, stream=stream)
        return outs, mem

    def chain(self, zero_udp=False):
        """The chain on copies of the same tensors, the READY subset gathered on
        the host for the build and scattered back: an expectation."""
        w, d, mem = self.w, self.d, self.fresh()
        c = SimpleNamespace(n=w.n, ndst=w.ndst, m=w.m)
        h = lambda t, dt=np.uint8: t.cpu().numpy().view(dt)  # noqa: E731
        state = None
        c.state, c.miss_list = np.zeros(0, np.uint8), np.zeros(0, np.uint32)
        c.sol_len, c.sol_built = np.zeros(w.m, np.uint16), 0
        if w.ndst:
            state, ml, mc = wc.tx_resolve(self.tab, mem.dsts, self.af)
            c.state, c.miss_list = h(state), h(ml, np.uint32)[:int(mc.item())]
            sl, sb = wc.tx_solicit_build(mem.dsts, self.af, ml, mc, self.eng, mem.sol, self.sol_offs,
                                         cases.SOL_SLOT)
            c.sol_len, c.sol_built = h(sl, np.uint16), int(sb.item())
        c.hold, c.held_list = np.zeros(0, np.uint8), np.zeros(0, np.uint32)
        c.status, c.errors = np.zeros(0, np.uint8), 0
        c.frame_len, c.ip_hdr, c.udp = (np.zeros(w.n, np.uint16) for _ in range(3))
        if w.n:
            hold, hl, hc = wc.tx_hold_plan(self.descs, self.socks, state, self.af)
            c.hold, c.held_list = h(hold), h(hl, np.uint32)[:int(hc.item())]
            ready = np.flatnonzero(c.hold == nmodel.TH_READY)
            c.status = np.where(c.hold == nmodel.TH_HELD, model.PUMP_HELD, bmodel.MALFORMED).astype(np.uint8)
            c.errors = int((c.hold == nmodel.TH_MALFORMED).sum())
            if ready.size:
                fl, st, ip, udp, err = wc.tx_build_ragged(
                    mem.buf, dev(w.offs[ready], d), dev_bytes(w.descs[ready], d), self.socks, mem.dsts,
                    w.slot, zero_udp=zero_udp)
                c.status[ready], c.frame_len[ready] = h(st), h(fl, np.uint16)
                c.ip_hdr[ready], c.udp[ready] = h(ip, np.uint16), h(udp, np.uint16)
                c.errors += int(err.item())
        torch.cuda.synchronize()
        c.dsts = h(mem.dsts).view(nmodel.DST) if w.ndst else np.zeros(0, nmodel.DST)
        c.buf, c.sol_out = h(mem.buf), h(mem.sol)
        return c


def check(o: Outs, mem, e, what: str, calls: int = 1):
    """The pump's fetched outputs and written tensors against an expectation."""
    for name, attr, dt in (("state", "state", np.uint8), ("hold", "hold", np.uint8),
                           ("status", "status", np.uint8), ("frame_lens", "frame_len", np.uint16),
                           ("ip_hdr", "ip_hdr", np.uint16), ("udp", "udp", np.uint16),
                           ("sol_lens", "sol_len", np.uint16)):
        got, want = o.get(name, dt), getattr(e, attr)
        assert got.shape == want.shape, (what, name)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, (what, name, bad[:8], got[bad[:8]], want[bad[:8]])
    for name, cname in LISTS.items():
        want, got = getattr(e, name), o.get(name, np.uint32)
        assert o.count(cname) == len(want), (what, cname, o.count(cname), len(want))
        np.testing.assert_array_equal(got[:len(want)], want, err_msg=f"{what} {name}")
        assert (got[len(want):] == 0xA5A5A5A5).all(), (what, name, "written past its count")
    assert o.count("sol_built") == e.sol_built, (what, "sol_built")
    assert o.count("errors") == ERRORS0 + calls * e.errors, (what, "errors", o.count("errors"), e.errors)
    if e.ndst:
        assert mem.dsts.cpu().numpy().tobytes() == e.dsts.tobytes(), (what, "the destination table")
    bad = np.flatnonzero(mem.buf.cpu().numpy() != e.buf)
    assert bad.size == 0, (what, "the frame buffer", bad[:8])
    bad = np.flatnonzero(mem.sol.cpu().numpy() != e.sol_out)
    assert bad.size == 0, (what, "the solicitation buffer", bad[:8])


def both_ways(d, w, zero_udp=False, tab=None):
    t = Dev(d, w, tab)
    o, mem = t.run(zero_udp)
    torch.cuda.synchronize()
    o.fetch()
    e = cases.expect(w, zero_udp)
    check(o, mem, e, "models")
    check(o, mem, t.chain(zero_udp), "chain")
    return o, e


PAIRS = [(1, 1), (63, 64), (64, 63), (65, 65), (600, 257), (SMALL - 1, SMALL_DST), (SMALL, SMALL_DST - 1),
         (SMALL, SMALL_DST), (SMALL + 1, 64), (64, SMALL_DST + 1), (600, 0), (0, 257)]


@pytest.mark.parametrize("n,ndst", PAIRS)
def test_both_ways_of_knowing_the_answer(gpu, n, ndst):
    """(4097, 64) and (64, 4097) take the fallback; 4095 / 4096: the plan
    workgroup's last partial and last full wave step."""
    k = PAIRS.index((n, ndst))
    layout = "slots" if n > 1000 else cases.LAYOUTS[k % 2]
    w = cases.world(100 + k, n, ndst, layout, connected_only=ndst == 0)
    o, e = both_ways(gpu, w, zero_udp=bool(k & 1))
    if n >= 600 and ndst >= 257:
        assert min(o.count(c) for c in LISTS.values()) > 0 and e.sol_built > 0 and e.errors > 0


@pytest.mark.parametrize("layout", cases.LAYOUTS)
@pytest.mark.parametrize("zero_udp", [False, True])
@pytest.mark.parametrize("m_delta", [-3, 0, 5])
def test_census_world_layouts_flag_and_m(gpu, layout, zero_udp, m_delta):
    """m below, at and above the miss count; both layouts; both flag values."""
    n, ndst = cases.CENSUS
    misses = len(cases.expect(cases.world(7, n, 0 + ndst, layout, m=0)).miss_list)
    assert misses >= 10
    w = cases.world(7, n, ndst, layout, m=misses + m_delta)
    o, e = both_ways(gpu, w, zero_udp)
    assert o.count("miss_count") == misses and e.sol_built == min(misses, w.m)


@pytest.mark.parametrize("m", [SMALL_DST, SMALL_DST + 1, 3 * SMALL_DST + 5])
def test_more_slots_than_destinations(gpu, m):
    """m at the small path's limit, and past it: a small batch then takes the
    chain's calls, which zero the unused lengths with a grid.  Every length past
    the miss count is 0 and every slot past it untouched either way."""
    w = cases.world(31, 65, 65, "pack_1_5", m=m)
    o, e = both_ways(gpu, w)
    misses = o.count("miss_count")
    assert 0 < misses == e.sol_built and not o.get("sol_lens", np.uint16)[misses:].any()


def big(seed=11, **kw):
    return cases.world(seed, SMALL, SMALL_DST, "slots", **kw)


def test_extreme_every_destination_resolved(gpu):
    w = big(nknown=512)
    good = [k for k in w.known if w.cache[nmodel.key(*k)] != nmodel.BCAST]
    rng = np.random.default_rng(1)
    picks = [good[int(i)] for i in rng.integers(0, len(good), SMALL_DST)]
    w.dsts = nc.dst_table([(a, 4000 + i) for i, (_, a) in enumerate(picks)], rng)
    w.afs = np.array([af for af, _ in picks], np.uint8)
    o, e = both_ways(gpu, w)
    assert not o.get("state").any() and o.count("miss_count") == 0 == o.count("held_count")
    assert (o.get("miss_list", np.uint32) == 0xA5A5A5A5).all() and o.count("sol_built") == 0
    assert (o.get("held_list", np.uint32) == 0xA5A5A5A5).all()
    assert not (o.get("status") == model.PUMP_HELD).any()
    unconnected = (w.descs["sock"] < 2) & (e.hold == nmodel.TH_READY) & (e.ungated == bmodel.SEALED)
    assert unconnected.sum() > 500 and (o.get("frame_lens", np.uint16)[unconnected] != 0).all()


def test_extreme_none_resolved_all_distinct(gpu):
    w = big()
    w.cache = {}
    ks = nc.keys(SMALL_DST)
    w.dsts = nc.dst_table([(a, 4000 + i) for i, (_, a) in enumerate(ks)], np.random.default_rng(2))
    w.afs = np.array([af for af, _ in ks], np.uint8)
    o, e = both_ways(gpu, w)
    assert (o.get("state") == nmodel.MISS).all() and o.count("miss_count") == SMALL_DST
    assert (o.get("miss_list", np.uint32) == np.arange(SMALL_DST)).all()
    assert o.count("sol_built") == SMALL_DST and (o.get("sol_lens", np.uint16)[:SMALL_DST] != 0).all()
    assert not o.get("sol_lens", np.uint16)[SMALL_DST:].any()
    hold = o.get("hold")
    assert (hold[(w.descs["sock"] < 2) & (hold != nmodel.TH_MALFORMED)] == nmodel.TH_HELD).all()
    assert o.count("held_count") > 500


def test_extreme_one_unresolved_address(gpu):
    w = big()
    w.cache = {}
    w.dsts = nc.dst_table([(nc.addr4(777) + bytes(12), 4000 + i) for i in range(SMALL_DST)],
                          np.random.default_rng(3))
    w.afs = np.full(SMALL_DST, 4, np.uint8)
    o, e = both_ways(gpu, w)
    state = o.get("state")
    assert state[0] == nmodel.MISS and (state[1:] == nmodel.MISS_DUP).all()
    assert o.count("miss_count") == 1 == o.count("sol_built") and o.get("miss_list", np.uint32)[0] == 0


def test_engine_table_without_an_ipv4_address(gpu):
    w = big(engine=rc.engine_table(v4=0))
    o, e = both_ways(gpu, w)
    lens = o.get("sol_lens", np.uint16)[:o.count("miss_count")]
    v4 = w.afs[e.miss_list] == 4
    assert v4.sum() > 10 and not lens[v4].any() and (lens[~v4] == nmodel.NSOL_LEN).all()


def test_a_table_never_initialised(gpu):
    w = big()
    w.cache = {}
    tab = torch.zeros(wc.neigh_tab_bytes(64), dtype=torch.uint8, device=gpu)
    o, e = both_ways(gpu, w, tab=tab)
    assert not (o.get("state") == nmodel.READY).any() and o.count("miss_count") > 100


def test_determinism_and_errors(gpu):
    for n, ndst in (cases.CENSUS, (SMALL, SMALL_DST)):
        w = cases.world(7, n, ndst, "slots")
        t, e = Dev(gpu, w), cases.expect(w)
        (a, ma), (b, mb) = t.run(), t.run()
        torch.cuda.synchronize()
        a.fetch(), b.fetch()
        for name in a.host:
            assert (a.host[name] == b.host[name]).all(), name
        for x in ("dsts", "buf", "sol"):
            assert torch.equal(getattr(ma, x), getattr(mb, x)), x
        assert e.errors > 0
        check(a, ma, e, "models")
        # accumulated: a second call on the same outputs and tensors adds the count again
        t.run(outs=a, mem=ma)
        torch.cuda.synchronize()
        check(a.fetch(), ma, e, "second call", calls=2)


def test_two_streams(gpu):
    """Two streams with their own scratch, outputs and tensors in one process,
    20 calls each on different worlds and sizes."""
    plan = [(cases.world(21, 600, 257, "pack_1_5"), True), (cases.world(22, SMALL, SMALL_DST, "slots"), False)]
    state = []
    for w, zero in plan:
        t = Dev(gpu, w)
        scratch = torch.empty(wc.tx_pump_scratch(w.n, w.ndst) // 4 + 1, dtype=torch.int32, device=gpu)
        state.append((t, zero, torch.cuda.Stream(gpu), scratch, t.fresh(),
                      [Outs(gpu, w.n, w.ndst, w.m) for _ in range(20)]))
    torch.cuda.synchronize()
    for k in range(20):
        for t, zero, st, scratch, mem, outs in state:
            t.run(zero, outs=outs[k], mem=mem, scratch=scratch, stream=st)
    torch.cuda.synchronize()
    for t, zero, st, scratch, mem, outs in state:
        e = cases.expect(t.w, zero)
        for o in outs:
            check(o.fetch(), mem, e, f"stream of n = {t.w.n}")


def test_empty_sides(gpu):
    # (0, 0) through the wrapper: the three counts, m zero lengths
    w = cases.world(5, 0, 0, m=4)
    o, e = both_ways(gpu, w)
    assert [o.count(c) for c in ("miss_count", "held_count", "sol_built")] == [0, 0, 0]
    assert not o.get("sol_lens", np.uint16).any() and o.count("errors") == ERRORS0
    # NULL everywhere but the three counts
    o = Outs(gpu, 0, 0, 0)
    members = dict(miss_count=o.out.miss_count, held_count=o.out.held_count, sol_built=o.out.sol_built)
    c_out = _PumpOut(**{k: t.data_ptr() for k, t in members.items()})
    rc_ = _lib.active().wc_tx_pump(None, None, None, 0, None, 0, None, 0, None, None, 0, 0, None, None,
                                   None, 0, 0, ctypes.byref(c_out), None,
                                   torch.cuda.current_stream(gpu).cuda_stream)
    torch.cuda.synchronize()
    o.fetch()
    assert rc_ == 0
    assert [o.count(c) for c in ("miss_count", "held_count", "sol_built")] == [0, 0, 0]
    for name in ("miss_list", "held_list"):
        assert (o.get(name, np.uint32) == 0xA5A5A5A5).all()


def rx_chain(d_buf, d_off, d_len, d_eng):
    """rx_verdict_ragged -> rx_reply_plan -> rx_neigh_plan over one ring."""
    v, _ = wc.rx_verdict_ragged(d_buf, d_off, d_len)
    act, _, _, _ = wc.rx_reply_plan(d_buf, d_off, d_len, v, None, d_eng, 2048, want_list=False)
    nact, rl, rcnt, ul, ucnt = wc.rx_neigh_plan(d_buf, d_off, d_len, act, d_eng)
    return act, nact, rl, rcnt, ul, ucnt


def test_closed_loop_with_the_pump(gpu):
    """test_gpu_tx_neigh's dozen peers with the pump in the place of the three
    calls and the build: round one HELD plus solicitations, the answers through
    rx_drain -> rx_neigh_updates -> neigh_apply, round two the same descriptors
    READY with tx_build_model's frames and the peers' MACs."""
    peers = nc.peers(12)
    eng = rc.engine_table()
    d_eng = dev_bytes(eng, gpu)
    dsts = nc.dst_table([(a4, 4433) for _, a4, _ in peers] + [(a6, 4433) for _, _, a6 in peers] +
                        [(peers[0][1], 4434), (peers[5][2], 4434)], np.random.default_rng(1))
    afs = np.array([4] * 12 + [6] * 12 + [4, 6], np.uint8)
    ndst = len(afs)
    socks = nc.socks_table()[:2]
    socks["lport"] = 0x5111
    descs = nc.descs_of([(0 if afs[t] == 4 else 1, t) for t in range(ndst)] * 3)
    n = len(descs)
    rng = np.random.default_rng(2)
    tx_off = np.arange(n, dtype=np.uint64) * 256 + 3
    tx0 = rng.integers(0, 256, n * 256 + 64, dtype=np.uint8)
    ring0, ring_off = rc.out_slots(ndst, 128, rng)
    d_dsts, d_af = dev_bytes(dsts, gpu), dev(afs, gpu)
    d_descs, d_socks = dev_bytes(descs, gpu), dev_bytes(socks, gpu)
    d_tx, d_tx_off = dev(tx0, gpu), dev(tx_off, gpu)
    d_ring, d_ring_off = dev(ring0, gpu), dev(ring_off, gpu)
    tab = wc.neigh_tab_init(64, gpu)

    def pump():
        return wc.tx_pump(tab, d_dsts, d_af, d_descs, d_socks, d_tx, d_tx_off, 256, d_eng, d_ring,
                          d_ring_off, 128)

    # round one: every frame HELD, untouched; 24 solicitations
    r = pump()
    assert r.state.cpu().tolist() == [wc.NR_MISS] * 24 + [wc.NR_MISS_DUP] * 2
    assert (r.hold.cpu().numpy() == wc.TH_HELD).all() and int(r.held_count.item()) == n
    assert (r.status.cpu().numpy() == wc.TX_PUMP_HELD).all() and int(r.errors.item()) == 0
    assert not r.frame_lens.cpu().numpy().view(np.uint16).any() and (d_tx.cpu().numpy() == tx0).all()
    assert int(r.sol_built.item()) == 24 == int(r.miss_count.item())
    want_ring, want_len, _ = nmodel.built(ring0, ring_off, 128, dsts, afs, np.arange(24), 24, eng)
    assert (d_ring.cpu().numpy() == want_ring).all()
    assert (r.sol_lens.cpu().numpy().view(np.uint16) == want_len).all()
    # each peer answers the two solicitations that ask for it
    reply0, reply_off = rc.out_slots(24, 128, rng)
    d_reply = dev(reply0, gpu)
    reply_len = torch.zeros(24, dtype=torch.uint16, device=gpu)
    for p, (mac, a4, a6) in enumerate(peers):
        d_peer = dev_bytes(nc.peer_engine(mac, a4, a6), gpu)
        _, nact, rl, rcnt, _, _ = rx_chain(d_ring, d_ring_off, r.sol_lens, d_peer)
        olen, built = wc.rx_neigh_build(d_ring, d_ring_off, r.sol_lens, nact, rl, rcnt, d_peer, d_reply,
                                        dev(reply_off[2 * p:2 * p + 2], gpu), 128)
        assert int(built.item()) == 2
        reply_len.view(torch.int16)[2 * p:2 * p + 2] = olen.view(torch.int16)
    # the answers: rx_drain -> rx_neigh_updates -> neigh_apply
    d_reply_off = dev(reply_off, gpu)
    sk = dcases.sockets(0, 1)
    dr = wc.rx_drain(d_reply, d_reply_off, reply_len, dev_bytes(wc.rx_socktab_build(sk), gpu), len(sk),
                     d_eng, 2048)
    assert int(dr.update_count.item()) == 24
    upd = wc.rx_neigh_updates(d_reply, d_reply_off, reply_len, dr.nact, dr.update_list, dr.update_count, 32)
    assert int(wc.neigh_apply(tab, upd, dr.update_count).item()) == 0
    # round two: the same descriptors, READY, with the peers' MACs
    r = pump()
    assert not r.state.cpu().numpy().any() and not r.hold.cpu().numpy().any()
    assert [int(x.item()) for x in (r.miss_count, r.held_count, r.sol_built, r.errors)] == [0, 0, 0, 0]
    after = d_dsts.cpu().numpy().view(nmodel.DST)
    macs = [p[0] for p in peers]
    assert [bytes(m) for m in after["dmac"]] == macs + macs + [macs[0], macs[5]]
    want = bmodel.Expect(tx0, tx_off, descs, socks, after, 256)
    tx = d_tx.cpu().numpy()
    assert (tx == want.buf).all() and (r.status.cpu().numpy() == wc.TX_SEALED).all()
    assert (r.frame_lens.cpu().numpy().view(np.uint16) == want.frame_len).all()
    for i in range(n):
        o = int(tx_off[i])
        assert tx[o:o + 6].tobytes() == macs[int(descs["dst"][i]) % 12 if descs["dst"][i] < 24
                                             else (0 if descs["dst"][i] == 24 else 5)]
    verdict, _ = wc.rx_verdict_ragged(d_tx, d_tx_off, r.frame_lens)
    assert (verdict.cpu().numpy() == wc.RX_OK).all()
