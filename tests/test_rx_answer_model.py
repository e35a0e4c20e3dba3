"""CPU tests of the RX answer worlds (tests/rx_answer_cases.py): the 600-frame
worlds the GPU tests run exercise every part of wc_rx_answer -- at least ten
frames of every reply action and of each of the four neighbour update / reply
codes, at least eight addresses per family that several records name with
different MACs, and at least one listed reply the build refuses -- and the
models' expectation of the answer is consistent with itself.  This keeps the
GPU test from passing on a world that exercises nothing."""
import numpy as np
import pytest

import rx_answer_cases as cases
import rx_drain_cases as dcases
import rx_neigh_model as nmodel
import rx_reply_cases as rc
import rx_reply_model as rmodel
import tx_neigh_model as tmodel
import warpcore_amd as wc


@pytest.fixture(scope="module", params=list(cases.WORLDS))
def planned(request):
    seed, n, ns, slot = cases.WORLDS[request.param]
    frames, socks = cases.world(seed, n, ns)
    tab = wc.rx_socktab_build(socks)
    buf, offs, lens = dcases.layout(request.param, frames, seed)
    eng = rc.engine_table(rng=np.random.default_rng(seed))
    return dcases.expect(buf, offs, lens, tab, ns, eng, slot), len(frames)


def test_constants():
    assert cases.SMALL == wc.RX_ANSWER_SMALL == 4096
    assert 86 <= cases.SLOT < min(s for _, _, _, s in cases.WORLDS.values())


def test_every_action_and_code_at_least_ten_times(planned):
    ex, n = planned
    assert n == cases.N == 600 == ex.n
    acts = ex.actions.tolist()
    for a in rmodel.REPLIES:
        assert acts.count(a) >= 10, ("reply action", a, acts.count(a))
    assert set(rmodel.REPLIES) == {wc.RR_ECHO4, wc.RR_ECHO6, wc.RR_UNREACH_PORT4,
                                   wc.RR_UNREACH_PORT6, wc.RR_UNREACH_PROTO4}
    codes = ex.nact.tolist()
    for c in (nmodel.UPDATE4, nmodel.ARP_IS_AT, nmodel.NADV, nmodel.UPDATE6):
        assert codes.count(c) >= 10, ("neighbour code", c, codes.count(c))


def test_last_wins_is_exercised_in_both_families(planned):
    ex, _ = planned
    count = len(ex.update_list)
    upd = ex.neigh.updates(count)
    keys = cases.contested(upd, count)
    assert len(keys[4]) >= 8 and len(keys[6]) >= 8, {af: len(k) for af, k in keys.items()}
    # and in order the last record's MAC is the one that stays
    cache = {}
    assert tmodel.apply(cache, upd, count, count) == 0
    u = upd.reshape(-1).view(tmodel.UPDATE).reshape(-1)
    for k in keys[4] + keys[6]:
        last = [j for j in range(count) if int(u["af"][j]) == k[0]
                and tmodel.key(k[0], bytes(u["addr"][j])) == k][-1]
        assert cache[k] == bytes(u["mac"][last])


def test_a_listed_reply_is_refused_by_the_build(planned):
    ex, _ = planned
    bad = cases.refused(ex)
    assert len(bad) >= 1
    rng = np.random.default_rng(3)
    out0, offs = rc.out_slots(len(ex.reply_list), cases.SLOT, rng)
    nout0, noffs = rc.out_slots(len(ex.neigh_reply_list), cases.SLOT, rng)
    a = cases.answer(ex, out0, offs, nout0, noffs, len(ex.update_list))
    for j, _ in bad:
        o = int(offs[j])
        assert a.r_len[j] == 0 and (a.r_out[o:o + cases.SLOT] == out0[o:o + cases.SLOT]).all()
    assert 0 < a.r_built == len(ex.reply_list) - len(bad)
    assert a.n_built == len(ex.neigh_reply_list) > 0  # an advertisement fits SLOT
    assert a.upd.any(axis=1).all() and a.dropped == 0


def test_subset_regroups_the_lists(planned):
    ex, n = planned
    idx = (np.arange(65) * 7 + 65) % n
    sub = cases.subset(ex, idx)
    assert sub.reply.list.tolist() == [i for i in range(65)
                                       if int(ex.actions[idx[i]]) in rmodel.REPLIES]
    assert set(sub.neigh.rlist.tolist()) <= set(sub.neigh.ulist.tolist())
    whole = cases.subset(ex, np.arange(n))
    assert (whole.reply.list == ex.reply_list).all() and (whole.neigh.ulist == ex.update_list).all()
