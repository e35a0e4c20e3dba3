"""GPU tests of the RX answer (wc_rx_answer): every output against the models'
expectation (tests/rx_answer_cases.answer: rx_reply_model, rx_neigh_model,
tx_neigh_model) AND against the chain it stands for -- rx_reply_build,
rx_neigh_updates, rx_neigh_build, neigh_apply -- run on identical tensors, bit
exact.  The plan in front is the real wc_rx_drain.  Every output is pre-filled
with 0xA5 between 64 guard bytes (so both built counts start as garbage), the
slots lie at every 16-byte phase in random-filled buffers that are compared
whole, *dropped starts at 7, and the RX buffer must be untouched.  The table is
compared through lookups, wc_neigh_tab_stats and the wc_tx_resolve view, never
byte for byte: which entry a key lands in may differ.

A frame's results depend on its bytes and the tables alone, so one expectation
per base world is computed once and every size is run as n offsets that point
at the same frames (test_gpu_rx_drain.World)."""
import numpy as np
import pytest
import torch

import rx_answer_cases as cases
import rx_drain_cases as dcases
import rx_neigh_cases as nc
import rx_reply_cases as rc
import tx_neigh_cases as tcases
import tx_neigh_model as tmodel
import warpcore_amd as wc
from test_gpu_rx_drain import World, dev, dev_bytes
from test_gpu_tx_neigh import check_table, host_view, lookups, want_lookups

pytestmark = pytest.mark.gpu

FILL, GUARD, DROPPED0 = 0xA5, 64, 7
SMALL, SLOT = cases.SMALL, cases.SLOT
ABSENT = [(4, tcases.addr4(9999)), (6, tcases.addr6(9999))]


class Guarded:
    """nbytes of 0xA5 between 64 guard bytes, viewed as dtype."""

    def __init__(self, d, nbytes: int, dtype=torch.uint8):
        self.nbytes = nbytes
        self.raw = torch.full((2 * GUARD + nbytes,), FILL, dtype=torch.uint8, device=d)
        self.view = self.raw[GUARD:GUARD + nbytes].view(dtype)

    def get(self, dtype=np.uint8) -> np.ndarray:
        h = self.raw.cpu().numpy()
        assert (h[:GUARD] == FILL).all() and (h[GUARD + self.nbytes:] == FILL).all(), "a guard"
        return h[GUARD:GUARD + self.nbytes].view(dtype)


class Case:
    """One call's tensors: the slots, the guarded outputs, and the inputs to run
    the answer or the chain on them."""

    def __init__(self, w: World, n: int, plan, d_off, d_len, r_m, n_m, u_m, seed=0, ids=False,
                 slot=SLOT, dropped=DROPPED0):
        d = w.d
        rng = np.random.default_rng(1000 * seed + r_m + 3 * n_m + 7 * u_m)
        self.w, self.n, self.plan, self.d_off, self.d_len = w, n, plan, d_off, d_len
        self.r_m, self.n_m, self.u_m, self.slot = r_m, n_m, u_m, slot
        self.r_out0, self.r_offs = rc.out_slots(r_m, slot, rng)
        self.n_out0, self.n_offs = rc.out_slots(n_m, slot, rng)
        self.ip_ids = rng.integers(0, 1 << 16, r_m).astype(np.uint16) if ids else None
        self.d_r_out, self.d_n_out = dev(self.r_out0.copy(), d), dev(self.n_out0.copy(), d)
        self.d_r_offs, self.d_n_offs = dev(self.r_offs, d), dev(self.n_offs, d)
        self.d_ids = dev(self.ip_ids, d) if ids else None
        self.g = {"reply_lens": Guarded(d, 2 * r_m, torch.uint16),
                  "reply_built": Guarded(d, 8, torch.int64),
                  "neigh_lens": Guarded(d, 2 * n_m, torch.uint16),
                  "neigh_built": Guarded(d, 8, torch.int64),
                  "updates": Guarded(d, 24 * u_m), "dropped": Guarded(d, 8, torch.int64)}
        self.g["dropped"].view.fill_(dropped)
        self.out = wc.RxAnswer(**{k: g.view for k, g in self.g.items()})
        self.out = self.out._replace(updates=self.out.updates.view(u_m, 24))

    def answer(self, tab=None, stream=None, scratch=None):
        wc.rx_answer(self.w.d_buf, self.d_off, self.d_len, self.plan, self.w.d_eng, self.d_r_out,
                     self.d_r_offs, self.d_n_out, self.d_n_offs, self.u_m, self.slot, self.d_ids,
                     tab, out=self.out, scratch=scratch, stream=stream)
        return self

    def fetch(self):
        torch.cuda.synchronize()
        g = self.g
        return dict(r_out=self.d_r_out.cpu().numpy(), n_out=self.d_n_out.cpu().numpy(),
                    r_len=g["reply_lens"].get(np.uint16), n_len=g["neigh_lens"].get(np.uint16),
                    r_built=int(g["reply_built"].get(np.uint64)[0]),
                    n_built=int(g["neigh_built"].get(np.uint64)[0]),
                    upd=g["updates"].get().reshape(self.u_m, 24),
                    dropped=int(g["dropped"].get(np.uint64)[0]))

    def chain(self, tab=None, dropped=DROPPED0):
        """The four calls on fresh copies of the same slots; everything on the host."""
        w, p, d = self.w, self.plan, self.w.d
        d_r_out, d_n_out = dev(self.r_out0.copy(), d), dev(self.n_out0.copy(), d)
        r_len, r_built = wc.rx_reply_build(w.d_buf, self.d_off, self.d_len, p.actions, p.reply_list,
                                           p.reply_count, w.d_eng, d_r_out, self.d_r_offs,
                                           self.slot, self.d_ids)
        upd = wc.rx_neigh_updates(w.d_buf, self.d_off, self.d_len, p.nact, p.update_list,
                                  p.update_count, self.u_m)
        n_len, n_built = wc.rx_neigh_build(w.d_buf, self.d_off, self.d_len, p.nact,
                                           p.neigh_reply_list, p.neigh_reply_count, w.d_eng,
                                           d_n_out, self.d_n_offs, self.slot)
        drop = torch.tensor([dropped], dtype=torch.int64, device=d)
        if tab is not None and self.u_m:
            wc.neigh_apply(tab, upd, p.update_count, self.u_m, drop)
        torch.cuda.synchronize()
        return dict(r_out=d_r_out.cpu().numpy(), n_out=d_n_out.cpu().numpy(),
                    r_len=r_len.cpu().numpy(), n_len=n_len.cpu().numpy(), r_built=int(r_built.item()),
                    n_built=int(n_built.item()), upd=upd.cpu().numpy().reshape(self.u_m, 24),
                    dropped=int(drop.item()))

    def models(self, cache=None, cap=None, dropped=DROPPED0):
        sub = cases.subset(self.w.base, self.w.index(self.n))
        a = cases.answer(sub, self.r_out0, self.r_offs, self.n_out0, self.n_offs, self.u_m, self.slot,
                         self.ip_ids, cache, cap)
        return dict(r_out=a.r_out, n_out=a.n_out, r_len=a.r_len, n_len=a.n_len, r_built=a.r_built,
                    n_built=a.n_built, upd=a.upd, dropped=dropped + a.dropped)


def same(got: dict, want: dict, what: str):
    for k, v in want.items():
        if isinstance(v, np.ndarray):
            assert got[k].shape == v.shape, (what, k, got[k].shape, v.shape)
            if v.size == 0:
                continue
            bad = np.flatnonzero((got[k] != v).reshape(len(v), -1).any(axis=1)) if v.ndim > 1 \
                else np.flatnonzero(got[k] != v)
            assert got[k].shape == v.shape and bad.size == 0, (what, k, bad[:8])
        else:
            assert got[k] == v, (what, k, got[k], v)


def drained(w: World, n: int):
    d_off, d_len = w.inputs(n)
    plan = w.run(n, d_off=d_off, d_len=d_len).out
    torch.cuda.synchronize()
    counts = [int(c.item()) for c in (plan.reply_count, plan.neigh_reply_count, plan.update_count)]
    return plan, d_off, d_len, counts


def both_ways(w, n, plan, d_off, d_len, r_m, n_m, u_m, ids=False, cap=64, seed=0):
    """One case through the answer, the chain and the models, each with a fresh
    table of `cap` entries; returns the answer's results and the models' cache."""
    c = Case(w, n, plan, d_off, d_len, r_m, n_m, u_m, seed, ids)
    tab_a, tab_c = wc.neigh_tab_init(cap, w.d), wc.neigh_tab_init(cap, w.d)
    got = c.answer(tab_a).fetch()
    cache = {}
    want = c.models(cache, cap)
    same(got, want, "models")
    same(got, c.chain(tab_c), "chain")
    assert (w.d_buf.cpu().numpy() == w.buf).all(), "the RX buffer was written"
    ks = [(af, a) for af, a in cache] + ABSENT
    if len(cache) < cap:  # (a full table: which new keys it keeps is unspecified)
        check_table(tab_a, cache, ks, cap)
        assert lookups(tab_a, ks) == lookups(tab_c, ks)
    return got, cache


@pytest.fixture(scope="module")
def worlds(gpu):
    out = {}
    for name, (seed, n, ns, slot) in cases.WORLDS.items():
        frames, socks = cases.world(seed, n, ns)
        out[name] = World(gpu, frames, socks, rc.engine_table(rng=np.random.default_rng(seed)), slot,
                          name, seed)
    return out


@pytest.mark.parametrize("layout", list(cases.WORLDS))
@pytest.mark.parametrize("n", [1, 63, 64, 65, 600, 4096])
def test_both_ways_of_knowing_the_answer(worlds, n, layout):
    """For each list with count c: m = c - 1, c and c + 5 (clamped at 0), with
    ip_id NULL and given; the cache in a table of 4096 entries."""
    w = worlds[layout]
    plan, d_off, d_len, (cr, cn, cu) = drained(w, n)
    if n >= 600:
        assert min(cr, cn, cu) > 0
    for k, delta in enumerate((-1, 0, 5)):
        m = [max(c + delta, 0) for c in (cr, cn, cu)]
        got, cache = both_ways(w, n, plan, d_off, d_len, *m, ids=k != 1, cap=4096, seed=n + k)
        if n >= 600 and delta == 0:
            assert 0 < got["r_built"] < cr and got["n_built"] == cn  # some echo finds no room
            assert got["dropped"] == DROPPED0 and len(cache) > 16


def tiled(gpu):
    """64 base frames, half of them echo requests and half requests for our
    addresses from sixteen hosts per family with changing MACs: every frame is in
    a list, 8320 frames put 4160 entries into each of the three."""
    rng = np.random.default_rng(77)
    frames = []
    for k in range(16):
        mac = bytes((2, 0, 0, 9, k % 4, int(rng.integers(0, 256))))
        frames.append(rc.echo4(bytes(int(rng.integers(0, 40)))))
        frames.append(nc.arp(tpa=nc.A4[k % 2], sha=mac, spa=bytes((192, 168, 78, 1 + k % 8))))
        frames.append(rc.echo6(bytes(int(rng.integers(0, 40)))))
        frames.append(nc.nd(135, nc.A6[k % 2], opt=b"\x01\x01" + mac,
                            src=nc.PEER6[:8] + bytes((0x78, 0, 0, 0, 0, 0, 0, 1 + k % 8))))
    return World(gpu, frames, dcases.sockets(6, 77), rc.engine_table(), 256, "packed", 5)


@pytest.fixture(scope="module")
def big(gpu):
    w = tiled(gpu)
    return (w,) + drained(w, 8320)


@pytest.mark.parametrize("ms", [(4095, 4096, 4096), (4096, 4095, 4095), (4095, 4096, 4097),
                                (4097, 9, 9), (9, 4097, 9), (9, 9, 1023), (9, 9, 1024),
                                (9, 9, 1025)])
def test_the_threshold_of_each_list(big, ms):
    """Every case here gives a table, so only those with u_m <= 1024 =
    RX_ANSWER_SMALL_APPLY run the two launches -- (4097, 9, 9) and (9, 4097, 9)
    aside -- and k_rx_answer_apply's claim and commit then use waves 0 to 3 of
    its 16; 1023 / 1024 are their last partial and last full step.  A 4097 in
    any of the three, and u_m = 1025, 4095, 4096 or 4097 with the table, take
    the chain's calls: there the answer is the chain, compared with the chain
    and the models.  The two launches at 4095 / 4096 entries per list run
    without a table in test_the_4096_tails_without_a_table."""
    w, plan, d_off, d_len, counts = big
    assert counts == [4160, 4160, 4160]
    got, cache = both_ways(w, 8320, plan, d_off, d_len, *ms, ids=True, cap=64, seed=sum(ms))
    assert got["r_built"] == ms[0] and got["n_built"] == ms[1] and len(cache) == min(16, ms[2])
    assert got["upd"].any(axis=1).all()


@pytest.mark.parametrize("ms", [(4095, 4096, 4096), (4096, 4095, 4095)])
def test_the_4096_tails_without_a_table(big, ms):
    """tab NULL: the two launches with 4095 / 4096 entries in every list -- the
    frames launch's last workgroups of each role, and step A of the apply
    workgroup over its last partial and last full wave step (B and C are
    skipped without a table)."""
    w, plan, d_off, d_len, _ = big
    c = Case(w, 8320, plan, d_off, d_len, *ms, seed=sum(ms), ids=True)
    got = c.answer(None).fetch()
    same(got, c.models(), "models")
    same(got, c.chain(None), "chain")
    assert (got["r_built"], got["n_built"], got["dropped"]) == (ms[0], ms[1], DROPPED0)
    assert got["upd"].any(axis=1).all()


def test_three_answers_in_a_row_on_one_table_and_no_table(worlds, gpu):
    w = worlds["slots"]
    tab_a, tab_c, cache = wc.neigh_tab_init(64, gpu), wc.neigh_tab_init(64, gpu), {}
    dropped = DROPPED0
    for n in (64, 65, 63):  # three rings, the same two tables
        plan, d_off, d_len, (cr, cn, cu) = drained(w, n)
        c = Case(w, n, plan, d_off, d_len, cr, cn, cu, seed=n, dropped=dropped)
        got = c.answer(tab_a).fetch()
        want = c.models(cache, 64, dropped)
        same(got, want, "models")
        same(got, c.chain(tab_c, dropped), "chain")
        dropped = got["dropped"]
        ks = list(cache) + ABSENT
        check_table(tab_a, cache, ks, 64)
        assert lookups(tab_a, ks) == lookups(tab_c, ks)
    assert len(cache) > 20
    # tab NULL: the table byte-identical, *dropped at 7
    before = host_view(tab_a).copy()
    plan, d_off, d_len, (cr, cn, cu) = drained(w, 600)
    c = Case(w, 600, plan, d_off, d_len, cr, cn, cu, seed=1)
    got = c.answer(None).fetch()
    same(got, c.models(), "models")
    same(got, c.chain(None), "chain")
    assert got["dropped"] == DROPPED0 and (host_view(tab_a) == before).all()


def ring_of(gpu, frames, eng=None, slot=256):
    return World(gpu, frames, dcases.sockets(6, 5), rc.engine_table() if eng is None else eng, slot,
                 "packed", len(frames) % 16)


@pytest.mark.parametrize("records", [wc.RX_ANSWER_SMALL_APPLY, SMALL])
def test_one_key_in_every_step_of_the_claiming_waves(gpu, records):
    """Records of two keys: a burst of ARP replies from one peer (and every 64th
    from a second) with changing MACs.  The last MAC wins, used == 2.  Only the
    1024 case runs k_rx_answer_apply -- one key in all four steps of waves 0 to
    3, the most a table lets the workgroup take; the 4096 case is above
    RX_ANSWER_SMALL_APPLY and runs the chain's calls, so it holds the fallback
    against the models."""
    frames = []
    for k in range(512):
        mac = bytes((2, 0, 1, k >> 8, k & 255, 7))
        spa = tcases.addr4(2) if k % 64 else tcases.addr4(3)
        frames.append(nc.arp(op=b"\x00\x02", sha=mac, spa=spa, tha=rc.MAC, dst=rc.MAC))
    w = ring_of(gpu, frames)
    plan, d_off, d_len, (cr, cn, cu) = drained(w, records)
    assert (cr, cn, cu) == (0, 0, records)
    got, cache = both_ways(w, records, plan, d_off, d_len, 0, 0, records)
    idx = w.index(records)
    last2 = max(i for i in range(records) if idx[i] % 64)
    last3 = max(i for i in range(records) if idx[i] % 64 == 0)
    assert cache == {(4, tcases.addr4(2)): frames[idx[last2]][22:28],
                     (4, tcases.addr4(3)): frames[idx[last3]][22:28]}
    assert got["dropped"] == DROPPED0 and got["r_built"] == 0 == got["n_built"]


def test_full_table_rule(gpu):
    """80 distinct peers, three ARP replies each with different MACs, into cap
    64: used == 64, every present key has its last MAC, dropped = the records of
    absent keys; no particular survivor set."""
    rng = np.random.default_rng(6)
    ks = [(4, tcases.addr4(100 + k)) for k in range(80)]
    frames = [nc.arp(op=b"\x00\x02", sha=tcases.mac_of(rng), spa=a, tha=rc.MAC, dst=rc.MAC)
              for _ in range(3) for _, a in ks]
    frames = [frames[i] for i in rng.permutation(len(frames))]
    w = ring_of(gpu, frames)
    n = len(frames)
    plan, d_off, d_len, (cr, cn, cu) = drained(w, n)
    assert cu == n == 240
    c = Case(w, n, plan, d_off, d_len, 0, 0, n)
    last = {}
    want = c.models(last)  # (no cap: every key's last MAC)
    for _ in range(2):
        c = Case(w, n, plan, d_off, d_len, 0, 0, n)
        tab = wc.neigh_tab_init(64, gpu)
        got = c.answer(tab).fetch()
        same({k: got[k] for k in ("upd", "r_built", "n_built")},
             {k: want[k] for k in ("upd", "r_built", "n_built")}, "models")
        look = lookups(tab, ks)
        assert sum(mac is not None for mac in look) == 64
        assert wc.neigh_tab_stats(host_view(tab)) == (64, 64)
        for k, mac in zip(ks, look):
            assert mac is None or mac == last[tmodel.key(*k)]
        absent = {tmodel.key(*k) for k, mac in zip(ks, look) if mac is None}
        u = want["upd"].reshape(-1).view(tmodel.UPDATE).reshape(-1)
        assert got["dropped"] == DROPPED0 + sum(
            tmodel.key(4, bytes(u["addr"][j])) in absent for j in range(n)) == DROPPED0 + 48


def test_stale_inputs(worlds, gpu):
    """An action byte overwritten with a non-reply code and list entries >= n:
    length 0, an untouched slot, a zero record -- and equality with the chain."""
    w = worlds["packed"]
    n = 600
    plan, d_off, d_len, (cr, cn, cu) = drained(w, n)
    ex = w.expect(n)
    act, nact = plan.actions.clone(), plan.nact.clone()
    rl, nrl, ul = plan.reply_list.clone(), plan.neigh_reply_list.clone(), plan.update_list.clone()
    stale_r, stale_n, stale_u = int(ex.reply_list[3]), int(ex.neigh_reply_list[2]), int(ex.update_list[5])
    act[stale_r] = wc.RR_FILTERED
    nact[stale_n] = wc.RN_NONE       # (its record and its reply both go)
    rl.view(torch.int32)[7], nrl.view(torch.int32)[4], ul.view(torch.int32)[9] = n, n + 5, -1
    stale = plan._replace(actions=act, nact=nact, reply_list=rl, neigh_reply_list=nrl, update_list=ul)
    c = Case(w, n, stale, d_off, d_len, cr, cn, cu, ids=True)
    tab_a, tab_c = wc.neigh_tab_init(4096, gpu), wc.neigh_tab_init(4096, gpu)
    got = c.answer(tab_a).fetch()
    same(got, c.chain(tab_c), "chain")
    jn = ex.neigh_reply_list.tolist().index(stale_n)
    for j, lens, out, out0, offs in ((3, "r_len", "r_out", c.r_out0, c.r_offs),
                                     (7, "r_len", "r_out", c.r_out0, c.r_offs),
                                     (jn, "n_len", "n_out", c.n_out0, c.n_offs),
                                     (4, "n_len", "n_out", c.n_out0, c.n_offs)):
        o = int(offs[j])
        assert got[lens][j] == 0 and (got[out][o:o + SLOT] == out0[o:o + SLOT]).all(), (lens, j)
    ju = ex.update_list.tolist().index(stale_n)
    assert not got["upd"][9].any() and not got["upd"][ju].any()
    assert got["upd"][5].any() == (stale_u != stale_n)
    ks = [(int(r[0]), bytes(r[8:24] if r[0] == 6 else r[8:12])) for r in got["upd"] if r[0]]
    assert lookups(tab_a, ks) == lookups(tab_c, ks)


def test_extreme_4096_echo_requests_of_1400_bytes(gpu):
    rng = np.random.default_rng(9)
    frames = [rc.echo4(rng.integers(0, 256, 1400, dtype=np.uint8).tobytes()) for _ in range(8)]
    w = ring_of(gpu, frames, slot=2048)
    plan, d_off, d_len, counts = drained(w, SMALL)
    assert counts == [SMALL, 0, 0]
    c = Case(w, SMALL, plan, d_off, d_len, SMALL, 0, 0, ids=True, slot=2048)
    got = c.answer(None).fetch()
    same(got, c.chain(None), "chain")
    same(got, c.models(), "models")
    assert got["r_built"] == SMALL and (got["r_len"] == 1442).all()


def test_extreme_all_arp_and_an_engine_without_ipv4(gpu):
    frames = [f[0] for f in nc.world(33, 66) if f[0][12:14] == b"\x08\x06"]
    assert len(frames) >= 20
    w = ring_of(gpu, frames)
    plan, d_off, d_len, (cr, cn, cu) = drained(w, SMALL)
    assert cr == 0 and cu > cn > 0
    got, _ = both_ways(w, SMALL, plan, d_off, d_len, 5, cn, cu, cap=4096)  # five reply slots, no reply
    assert got["r_built"] == 0 and not got["r_len"].any() and got["n_built"] == cn
    # without an IPv4 address no ARP frame is looked at (eth.c:80): three empty lists
    w = ring_of(gpu, frames, rc.engine_table(v4=0))
    plan, d_off, d_len, counts = drained(w, 600)
    assert counts == [0, 0, 0]
    got, cache = both_ways(w, 600, plan, d_off, d_len, 5, 5, 5)
    assert not got["upd"].any() and not cache and got["n_built"] == 0


def test_all_m_zero_and_no_frame(worlds, gpu):
    w = worlds["slots"]
    plan, d_off, d_len, _ = drained(w, 600)
    got, _ = both_ways(w, 600, plan, d_off, d_len, 0, 0, 0)
    assert got["r_built"] == 0 == got["n_built"] and got["dropped"] == DROPPED0
    # n == 0 with m > 0: zero lengths, zero records, untouched slots
    plan, d_off, d_len, counts = drained(w, 0)
    assert counts == [0, 0, 0]
    for ms in ((3, 4, 5), (SMALL + 1, 4, 5)):
        c = Case(w, 0, plan, d_off, d_len, *ms)
        tab = wc.neigh_tab_init(64, gpu)
        got = c.answer(tab).fetch()
        same(got, c.chain(wc.neigh_tab_init(64, gpu)), "chain")
        assert not got["r_len"].any() and not got["n_len"].any() and not got["upd"].any()
        assert (got["r_out"] == c.r_out0).all() and (got["n_out"] == c.n_out0).all()
        assert (got["r_built"], got["n_built"], got["dropped"]) == (0, 0, DROPPED0)
        assert wc.neigh_tab_stats(host_view(tab)) == (64, 0)


@pytest.mark.parametrize("n", [2048, SMALL])
def test_determinism(worlds, gpu, n):
    """2048 frames: some 540 records, the two launches; 4096: more than
    RX_ANSWER_SMALL_APPLY records with a table, the chain's calls."""
    w = worlds["packed"]
    plan, d_off, d_len, (cr, cn, cu) = drained(w, n)
    assert (cu <= wc.RX_ANSWER_SMALL_APPLY) == (n == 2048)
    runs = []
    for _ in range(2):
        c = Case(w, n, plan, d_off, d_len, cr, cn, cu, ids=True)
        tab = wc.neigh_tab_init(4096, gpu)
        got = c.answer(tab).fetch()
        ks = [(int(r[0]), bytes(r[8:24] if r[0] == 6 else r[8:12])) for r in got["upd"]]
        runs.append((got, lookups(tab, ks), wc.neigh_tab_stats(host_view(tab))))
    same(runs[0][0], runs[1][0], "second run")
    assert runs[0][1:] == runs[1][1:] and None not in runs[0][1]


def test_two_streams(worlds, gpu):
    """Two streams with their own outputs, scratch and table, 20 calls each
    (both on the two launches: 159 and some 540 records)."""
    state = []
    for name, n in (("slots", 600), ("packed", 2048)):
        w = worlds[name]
        plan, d_off, d_len, (cr, cn, cu) = drained(w, n)
        calls = [Case(w, n, plan, d_off, d_len, cr, cn, cu, ids=True) for _ in range(20)]
        scratch = torch.empty(max(1, wc.rx_answer_scratch(cu) // 4), dtype=torch.int32, device=gpu)
        state.append((calls, wc.neigh_tab_init(4096, gpu), torch.cuda.Stream(gpu), scratch))
    torch.cuda.synchronize()
    for k in range(20):
        for calls, tab, st, scratch in state:
            calls[k].answer(tab, stream=st, scratch=scratch)
    torch.cuda.synchronize()
    for calls, tab, st, scratch in state:
        cache = {}
        want = calls[0].models(cache, 4096)
        assert want["dropped"] == DROPPED0
        for c in calls:
            same(c.fetch(), want, "stream")
        check_table(tab, cache, list(cache) + ABSENT, 4096)


def test_closed_loop_drain_answer_pump(gpu):
    """A ring of the peers' ARP replies and neighbour advertisements, then a TX
    batch to those peers: drain -> answer -> pump on one stream with no host
    read in between builds every frame with its peer's MAC, and the pump's
    frames, statuses and solicitations equal those of the same ring taken
    through the chain's calls (test_gpu_tx_neigh.test_closed_loop_on_the_device's
    world: a dozen peers in both families, two repeated destinations, and two
    destinations nobody answered for)."""
    peers = tcases.peers(12)
    eng = rc.engine_table()
    frames = []
    for mac, a4, a6 in peers:
        frames.append(nc.arp(op=b"\x00\x02", sha=mac, spa=a4, tha=rc.MAC, dst=rc.MAC, src=mac))
        # (icmp6.c:295-304 reads a type-1 option, else eth->src -- rx_neigh_model._nd_mac)
        frames.append(nc.nd(136, a6, opt=b"\x01\x01" + mac, src=a6, dst=nc.A6[0], eth_dst=rc.MAC))
    w = World(gpu, frames, dcases.sockets(6, 5), eng, 256, "packed", 3)
    n = len(frames)
    d_off, d_len = w.inputs(n)
    dsts = tcases.dst_table([(a4, 4433) for _, a4, _ in peers] + [(a6, 4433) for _, _, a6 in peers]
                            + [(peers[0][1], 4434), (peers[5][2], 4434),
                               (tcases.addr4(9999), 4433), (tcases.addr6(9999), 4433)],
                            np.random.default_rng(1))
    afs = np.array([4] * 12 + [6] * 12 + [4, 6, 4, 6], np.uint8)
    ndst = len(afs)
    socks = tcases.socks_table()[:2]
    socks["lport"] = 0x5111
    descs = tcases.descs_of([(0 if afs[t] == 4 else 1, t) for t in range(ndst)] * 3)
    nf = len(descs)
    rng = np.random.default_rng(2)
    tx0 = rng.integers(0, 256, nf * 256 + 64, dtype=np.uint8)
    tx_off = np.arange(nf, dtype=np.uint64) * 256 + 3
    sol0, sol_off = rc.out_slots(ndst, 128, rng)
    d_descs, d_socks, d_af = dev_bytes(descs, gpu), dev_bytes(socks, gpu), dev(afs, gpu)
    d_tx_off, d_sol_off = dev(tx_off, gpu), dev(sol_off, gpu)

    def turn(answer: bool):
        tab = wc.neigh_tab_init(64, gpu)
        d_dsts, d_tx, d_sol = dev_bytes(dsts, gpu), dev(tx0.copy(), gpu), dev(sol0.copy(), gpu)
        st = torch.cuda.Stream(gpu)
        torch.cuda.synchronize()
        with torch.cuda.stream(st):
            plan = w.run(n, stream=st, d_off=d_off, d_len=d_len).out
            c = Case(w, n, plan, d_off, d_len, 4, 4, 32)
            if answer:
                c.answer(tab, stream=st)
                upd, dropped = c.out.updates, c.out.dropped
            else:
                upd = wc.rx_neigh_updates(w.d_buf, d_off, d_len, plan.nact, plan.update_list,
                                          plan.update_count, 32, stream=st)
                dropped = wc.neigh_apply(tab, upd, plan.update_count, 32, stream=st)
            p = wc.tx_pump(tab, d_dsts, d_af, d_descs, d_socks, d_tx, d_tx_off, 256, w.d_eng, d_sol,
                           d_sol_off, 128, stream=st)
        torch.cuda.synchronize()
        h = lambda t: t.cpu().numpy()  # noqa: E731
        return dict(tx=h(d_tx), sol=h(d_sol), dsts=h(d_dsts), status=h(p.status), state=h(p.state),
                    frame_lens=h(p.frame_lens), sol_lens=h(p.sol_lens), hold=h(p.hold),
                    sol_built=int(p.sol_built.item()), held=int(p.held_count.item()),
                    upd=h(upd).reshape(32, 24)), tab

    got, tab = turn(True)
    want, tab_c = turn(False)
    same(got, want, "chain")
    after = got["dsts"].view(tmodel.DST)
    macs = [p[0] for p in peers]
    assert [bytes(m) for m in after["dmac"][:26]] == macs + macs + [macs[0], macs[5]]
    assert got["state"].tolist() == [wc.NR_READY] * 26 + [wc.NR_MISS] * 2
    assert got["sol_built"] == 2 and got["held"] == 6
    status = got["status"].reshape(3, ndst)
    assert (status[:, :26] == wc.TX_SEALED).all() and (status[:, 26:] == wc.TX_PUMP_HELD).all()
    for i in range(nf):
        if i % ndst < 26:
            o = int(tx_off[i])
            assert got["tx"][o:o + 6].tobytes() == macs[(i % ndst) % 12 if i % ndst < 24
                                                        else (0 if i % ndst == 24 else 5)]
    assert wc.neigh_tab_stats(host_view(tab)) == (64, 24) == wc.neigh_tab_stats(host_view(tab_c))
    assert want_lookups({}, ABSENT) == lookups(tab, ABSENT)
