"""The boundary grid of tests/rx_edges.py on the CPU: both oracles agree on
every frame, and the grid stands on each side of every threshold of the
decision chains -- per header shape, by construction, with no tolerance: an
empty bin is a bug in the generator.  (The GPU runs of the same grid are in
test_gpu_rx_edges.py, the comparison with the reference in test_reference.py.)
"""
import numpy as np
import pytest

import rx_deliver_model as deliver_model
import rx_edges
import tx_model
from oracle import py_oracle
from rx_edges import BAD_UDP, OK, OK_NO_CKSUM, TRUNCATED

SHAPE_NAMES = [rx_edges.shape_name(s) for s in rx_edges.SHAPES]
BASE_NAMES = [rx_edges.shape_name(s) for s in rx_edges.LADDER_BASES]


@pytest.fixture(scope="module")
def grid():
    return rx_edges.grid()


@pytest.fixture(scope="module")
def verdicts(grid):
    v = rx_edges.oracle_verdicts(grid)
    v.setflags(write=False)
    return v


@pytest.fixture(scope="module")
def census(grid, verdicts):
    c = rx_edges.census(grid, verdicts)
    print(rx_edges.census_table(c))
    return c


def count(census, decision, dist, shape, verdict=None) -> int:
    return sum(n for (d, k, s, v), n in census.items()
               if d == decision and k == dist and s == shape and verdict in (None, v))


def test_grid_is_small_and_deterministic(grid):
    assert 5000 < len(grid) < 12000
    assert all(0 <= flen <= len(fr) < 128 for fr, flen, _ in grid)
    assert len({tag for _, _, tag in grid}) == len(grid)  # a tag names one frame
    rx_edges.grid.cache_clear()
    try:
        assert rx_edges.grid() == grid
    finally:
        rx_edges.grid.cache_clear()


def test_both_oracles_agree_on_every_frame(grid, verdicts):
    py = np.array([py_oracle.rx_verdict(fr, flen) for fr, flen, _ in grid], np.uint8)
    bad = np.flatnonzero(py != verdicts)
    assert bad.size == 0, (f"{bad.size} frames, first {grid[bad[0]][2]}: c_oracle "
                           f"{verdicts[bad[0]]} py_oracle {py[bad[0]]}")
    assert set(np.unique(verdicts).tolist()) == set(range(10))


@pytest.mark.parametrize("shape", SHAPE_NAMES)
def test_every_shape_stands_on_both_sides_of_every_threshold(census, shape):
    for dist in (-1, 0, 1):  # flen 13 | 14 | 15
        assert count(census, "flen", dist, shape) >= 1, ("flen", dist)
    assert count(census, "flen", -1, shape, TRUNCATED) == count(census, "flen", -1, shape)
    for decision in ("hdr", "ip_plen", "udp_hdr"):
        for dist in (-1, 0):
            assert count(census, decision, dist, shape) >= 1, (decision, dist)
    # one byte short of the header / of the UDP header: nothing but TRUNCATED
    for decision in ("hdr", "udp_hdr"):
        assert count(census, decision, -1, shape, TRUNCATED) == count(census, decision, -1, shape)
    assert count(census, "ip_plen", -1, shape, py_oracle.RX_SHORT) \
        == count(census, "ip_plen", -1, shape)
    # the checked range ends one past the frame, on its last byte, one before it
    assert count(census, "range", -1, shape, TRUNCATED) == count(census, "range", -1, shape) >= 1
    for dist in (0, 1):
        assert count(census, "range", dist, shape, OK) >= 1, ("range", dist, "OK")
        assert count(census, "range", dist, shape, BAD_UDP) >= 1, ("range", dist, "BAD_UDP")


@pytest.mark.parametrize("shape", BASE_NAMES)
def test_field_ladder_bases_stand_on_both_sides_of_min_and_ulen(grid, verdicts, census, shape):
    for dist in (-1, 0, 1):  # ulen == ip_plen - 1 | ip_plen | ip_plen + 1
        assert count(census, "min", dist, shape) >= 1, ("min", dist)
    for dist in (-1, 0):     # ulen 7 | 8
        for v in (OK, OK_NO_CKSUM):
            assert count(census, "ulen", dist, shape, v) >= 1, ("ulen", dist, v)
    # the record's documented wrap and its documented indifference to the slot length
    big = {OK: 0, OK_NO_CKSUM: 0}
    past = 0
    for (fr, flen, _), v in zip(grid, verdicts.tolist()):
        if v in big and rx_edges.frame_shape(fr) == shape:
            r = deliver_model.record_of(fr, flen, v)
            big[v] += int(r["data_len"]) >= 65528
            past += v == OK_NO_CKSUM and int(r["data_off"]) + int(r["data_len"]) > flen
    assert big[OK] >= 1 and big[OK_NO_CKSUM] >= 1 and past >= 1, (big, past)


def test_unshifted_chain_is_the_oracles(grid, verdicts):
    got = np.array([rx_edges.shifted_chain(fr, flen) for fr, flen, _ in grid], np.uint8)
    bad = np.flatnonzero(got != verdicts)
    assert bad.size == 0, (grid[bad[0]][2], got[bad[0]], verdicts[bad[0]])


@pytest.mark.parametrize("which,by", rx_edges.WRONG_CHAINS)
def test_grid_tells_every_off_by_one_from_the_oracle(grid, verdicts, which, by):
    """A chain with one comparison off by one (either way), with MIN() dropped,
    or reading one byte past the frame differs from the oracle on grid frames
    of every header shape: a kernel copy with that slip cannot pass
    test_gpu_rx_edges.py, whichever parse the shape takes."""
    caught = {rx_edges.frame_shape(fr) for (fr, flen, _), v in zip(grid, verdicts.tolist())
              if rx_edges.shifted_chain(fr, flen, which, by) != v}
    need = set(BASE_NAMES) if which == "min" else set(SHAPE_NAMES)
    if which == "flen":  # flen 13 | 14 | 15 decides before there is a shape: for an IP
        need = {"other"}  # frame room < 1 follows, only another EtherType shows it
    assert need <= caught, sorted(need - caught)


@pytest.fixture(scope="module")
def tx_status(grid):
    """The seal model's status codes, without and with zero_udp."""
    return {z: tx_model.Expect(*rx_edges.packed(grid), zero_udp=z).status for z in (False, True)}


@pytest.mark.parametrize("zero_udp", [False, True])
def test_unshifted_seal_chain_is_the_models(grid, tx_status, zero_udp):
    got = np.array([rx_edges.shifted_seal_status(fr, flen, zero_udp) for fr, flen, _ in grid],
                   np.uint8)
    bad = np.flatnonzero(got != tx_status[zero_udp])
    assert bad.size == 0, (grid[bad[0]][2], got[bad[0]], tx_status[zero_udp][bad[0]])


@pytest.mark.parametrize("which,by", rx_edges.TX_WRONG_CHAINS)
def test_grid_tells_every_off_by_one_seal_from_the_model(grid, tx_status, which, by):
    """The same for tx_decide: one comparison of the seal's chain off by one,
    or MIN() dropped, changes the status of grid frames of every shape, in
    one of the two runs (zero_udp off and on) test_gpu_rx_edges.py makes."""
    caught = {rx_edges.frame_shape(fr) for z in (False, True)
              for (fr, flen, _), s in zip(grid, tx_status[z].tolist())
              if rx_edges.shifted_seal_status(fr, flen, z, which, by) != s}
    need = set(SHAPE_NAMES)
    if which == "flen":
        need = {"other"}
    if which == "ihl":  # hl < 21: only IHL 5 is at the threshold
        need = {"ihl5"}
    if which == "min" or (which, by) == ("ulen", -1):  # udp_len 7: the field ladder's bases
        need = set(BASE_NAMES)
    assert need <= caught, sorted(need - caught)


def test_small_ihl_frames_reach_the_udp_sum(grid, verdicts):
    """IHL 2..4 with a passing header sum: OK and BAD_UDP both occur, and for
    hl 12 and 16 also where udp_len + hl < 20 (payload_cksum's pseudo-header
    reads run past its len).  IHL 0 and 1 never pass ip_cksum(ip, hl)."""
    seen = set()
    for (fr, flen, tag), v in zip(grid, verdicts.tolist()):
        if not tag.startswith("ihlsmall/"):
            continue
        hl = (fr[14] & 0x0F) * 4
        assert hl < 20
        if hl < 8:
            assert v in (TRUNCATED, py_oracle.RX_BAD_IP_CKSUM), tag
        elif v in (OK, BAD_UDP):
            ulen = (fr[14 + hl + 4] << 8) | fr[14 + hl + 5]
            ip_plen = (((fr[16] << 8) | fr[17]) - hl) & 0xFFFF
            seen.add((hl, v, min(ulen, ip_plen) + hl < 20))
    assert {(hl, v, False) for hl in (8, 12, 16) for v in (OK, BAD_UDP)} <= seen
    assert {(hl, v, True) for hl in (12, 16) for v in (OK, BAD_UDP)} <= seen


def test_every_tx_status_occurs_and_a_cut_udp_header_stores_nothing(grid):
    frames = rx_edges.garbled(grid)
    buf, offs, lens = rx_edges.packed(frames)
    plain = tx_model.Expect(buf, offs, lens)
    zero = tx_model.Expect(buf, offs, lens, zero_udp=True)
    assert set(np.unique(plain.status).tolist()) == set(range(8)) - {tx_model.SEALED_ZERO_UDP}
    assert set(np.unique(zero.status).tolist()) == set(range(8)) - {tx_model.SEALED}
    cut, at_ulen = set(), set()
    for (fr, flen, tag), s, z in zip(frames, plain.seals, zero.seals):
        shape = rx_edges.frame_shape(fr)
        if tag.startswith("field/") and tag.endswith("/trailer=1"):
            # udp_len 7 | 8 in the seal, the UDP header inside the frame
            p, u = (int(x.split("=")[1]) for x in tag.split("/")[3:5])
            if p >= 8 and min(u, p) in (7, 8):
                at_ulen.add((shape, min(u, p), s.status, z.status))
        if tag.startswith("cut/") and shape != "none":
            hl = 40 if shape == "v6" else 4 * int(shape[3:])
            if flen == 14 + hl + 7:  # one byte short of the UDP header
                assert (s.status, z.status) == (tx_model.TRUNCATED, tx_model.TRUNCATED), tag
                assert s.stores == z.stores == (), tag
                cut.add(shape)
    assert cut == set(SHAPE_NAMES)
    for shape in BASE_NAMES:
        assert {(a, b) for sh, k, a, b in at_ulen if sh == shape and k == 7} \
            == {(tx_model.MALFORMED, tx_model.MALFORMED)}
        assert {(a, b) for sh, k, a, b in at_ulen if sh == shape and k == 8} \
            == {(tx_model.SEALED, tx_model.SEALED_ZERO_UDP)}
