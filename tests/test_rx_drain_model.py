"""CPU tests of the RX drain worlds (tests/rx_drain_cases.py): the 600-frame
worlds the GPU tests run hold at least ten frames of every class of the three
censuses the chain's own tests keep -- every socket id with NONE and UNBOUND
(test_gpu_rx_demux.py), every reply action (test_rx_reply_model.py), every
neighbour (code, cause) of rx_neigh_cases.CENSUS -- and the expected lists are
consistent with each other.  This keeps the GPU test from passing on a world
that exercises nothing."""
import numpy as np
import pytest

import rx_demux_model as xmodel
import rx_drain_cases as cases
import rx_neigh_cases as nc
import rx_neigh_model as nmodel
import rx_reply_cases as rc
import rx_reply_model as rmodel

# (NONE, "not nd") needs a HOST action byte on an IPv6 frame that is no
# neighbour discovery: wc_rx_reply_plan gives none (its chain names HOST on an
# IPv6 frame only for ICMPv6 types 135 / 136), so behind the real plan -- the
# drain has no other -- the class is empty; rx_neigh_cases forces such bytes.
NEIGH_CENSUS = [k for k in nc.CENSUS if k != (nmodel.NONE, "not nd")]


@pytest.fixture(scope="module", params=list(cases.WORLDS))
def planned(request):
    seed, n, ns, slot = cases.WORLDS[request.param]
    frames, socks = cases.world(seed, n, ns)
    tab = cases.wc.rx_socktab_build(socks)
    buf, offs, lens = cases.layout(request.param, frames, seed)
    eng = rc.engine_table(rng=np.random.default_rng(seed))
    return cases.expect(buf, offs, lens, tab, ns, eng, slot), ns, socks


def test_socket_table_is_over_the_engines_addresses(planned):
    _, ns, socks = planned
    assert len(socks) == ns and xmodel.valid(socks)
    assert bytes(socks[0]["laddr"][:4]) == rc.A4[0] and bytes(socks[1]["laddr"]) == rc.A6[0]


def test_every_census_class_at_least_ten_times(planned):
    ex, ns, _ = planned
    ids = ex.sock.tolist()
    for s in list(range(ns)) + [xmodel.NONE, xmodel.UNBOUND]:
        assert ids.count(s) >= 10, ("socket", s, ids.count(s))
    acts = ex.actions.tolist()
    for a in rmodel.ALL_ACTIONS:
        assert acts.count(a) >= 10, ("action", a, acts.count(a))
    c = ex.neigh.census()
    assert set(c) == set(NEIGH_CENSUS)
    for key in NEIGH_CENSUS:
        assert c[key] >= 10, (key, c[key])
    assert set(ex.verdicts.tolist()) >= {0, 1, 3, 5, 7, 8}  # delivered, both drops, host


def test_expected_lists_agree_with_each_other(planned):
    ex, ns, _ = planned
    n = ex.n
    assert all(int(ex.actions[i]) in rmodel.REPLIES for i in ex.reply_list)
    assert all(int(ex.reply_lens[i]) > 0 for i in ex.reply_list)
    assert int(ex.start[255]) == int(np.isin(ex.verdicts, (0, 1)).sum()) == len(ex.list)
    assert sorted(ex.list.tolist()) == np.flatnonzero(ex.sock != xmodel.NONE).tolist()
    for s in range(ns):
        run = ex.list[int(ex.start[s]):int(ex.start[s + 1])]
        assert (ex.sock[run] == s).all() and (np.diff(run.astype(np.int64)) > 0).all()
    assert (ex.start[ns:255] == ex.start[ns]).all()
    assert set(ex.neigh_reply_list.tolist()) <= set(ex.update_list.tolist())
    assert all(int(ex.actions[i]) == rmodel.HOST for i in ex.update_list)
    assert (ex.records["af"] != 0).sum() == len(ex.list)
    assert ex.drops == int(np.isin(ex.verdicts, (2, 3, 4, 5, 6, 9)).sum()) > 0
    assert 0 < len(ex.reply_list) < n and 0 < len(ex.neigh_reply_list) < len(ex.update_list) < n


def test_small_worlds_keep_their_size_and_mix():
    for n in (1, 63, 65, 129):
        frames, socks = cases.world(500 + n, n, 6)
        assert len(frames) == n and len(socks) == 6
    a, _ = cases.world(7, 129, 6)
    b, _ = cases.world(7, 129, 6)
    assert a == b  # seeded
