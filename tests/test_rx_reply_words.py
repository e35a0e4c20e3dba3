"""CPU test of the lines the RX reply kernels compile
(warpcore_amd/csrc/wc_rx_reply.h), compiled for the host alone
(tests/c/rx_reply_words.cpp): chain codes, reply lengths and reply bytes
against tests/rx_reply_model.py at all 16 byte phases of source and
destination.  The program itself refuses a load that does not overlap the
frame and a store that is misaligned or leaves the reply."""
import struct
import subprocess

import numpy as np
import pytest

import cprog
import rx_reply_cases as cases
import rx_reply_model as model
from oracle import c_oracle

REGION = 2304
OWN = 0xFFFFFFFF


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return cprog.build_words("rx_reply_words", tmp_path_factory.mktemp("rxr"))


def run(exe, tmp_path, items):
    """items: (frame, verdict, sock or None, engine, slot_bytes, action or OWN,
    ip_id, source phase, destination phase) -> [(action, reply_len, out_len,
    region bytes)]."""
    blob = bytearray()
    for fr, verdict, sock, eng, slot, act, ip_id, sp, dp in items:
        blob += eng.tobytes()
        blob += struct.pack("<8I", verdict, 0x100 if sock is None else sock, slot, act, ip_id, sp,
                            dp, len(fr))
        blob += fr
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(bytes(blob))
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = dst.read_bytes()
    rec = 12 + REGION
    assert len(raw) == len(items) * rec
    return [struct.unpack("<3I", raw[i:i + 12]) + (raw[i + 12:i + rec],)
            for i in range(0, len(raw), rec)]


def want_of(fr, verdict, sock, eng, slot, act, ip_id, dp):
    a, ln = model.plan(fr, verdict, sock, eng, slot)
    use = a if act == OWN else act
    reply = model.build(fr, use, eng, ip_id) if use in model.REPLIES else None
    if reply is not None and len(reply) > slot:
        reply = None
    region = bytearray(b"\xa5" * REGION)
    if reply is not None:
        region[16 + dp:16 + dp + len(reply)] = reply
    return a, ln, len(reply) if reply is not None else 0, bytes(region)


def check(exe, tmp_path, items):
    got = run(exe, tmp_path, items)
    for i, (g, it) in enumerate(zip(got, items)):
        fr, verdict, sock, eng, slot, act, ip_id, sp, dp = it
        w = want_of(fr, verdict, sock, eng, slot, act, ip_id, dp)
        assert g[:3] == w[:3], f"case {i}: phases {sp}/{dp}, action {act}"
        assert g[3] == w[3], f"case {i}: phases {sp}/{dp}: reply bytes"
    return got


def test_grid_every_phase(exe, tmp_path):
    grid = cases.grid()
    items = []
    for k in range(16):
        for j, (name, fr, sock, eng, slot, act, ln) in enumerate(grid):
            items.append((fr, c_oracle.rx_verdict(fr, len(fr)), sock, eng, slot, OWN, 0x1234 + j,
                          k, (5 * k + j) % 16))
    got = check(exe, tmp_path, items)
    for g, (name, fr, sock, eng, slot, act, ln) in zip(got, grid * 16):
        assert g[:3] == (act, ln, ln), name


@pytest.mark.parametrize("sp", range(16))
def test_echo_lengths_every_source_and_destination_phase(exe, tmp_path, sp):
    rng = np.random.default_rng(sp)
    eng = cases.engine_table(rng=rng)
    items = []
    for dp in range(16):
        for dl in (0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 33, 64, 257):
            data = rng.integers(0, 256, dl, dtype=np.uint8).tobytes()
            for fr in (cases.echo4(data), cases.echo6(data),
                       cases.echo4(data, ihl=int(rng.integers(6, 16)), rng=rng)):
                items.append((fr, model.RX_NOT_UDP, None, eng, 2048, OWN,
                              int(rng.integers(0, 1 << 16)), sp, dp))
    got = check(exe, tmp_path, items)
    assert all(g[2] != 0 for g in got)


def test_world_and_unreachables(exe, tmp_path):
    seed, n, slot = cases.WORLDS["slots"]
    frames = cases.world(seed, n)
    v, sk = cases.verdicts_of(frames), cases.socks_of(frames)
    eng = cases.engine_table()
    items = [(fr, int(v[i]), int(sk[i]), eng, slot, OWN, i, i % 16, (i // 16) % 16)
             for i, (fr, _) in enumerate(frames)]
    items += [(fr, int(v[i]), None, eng, slot, OWN, i, 3, 9) for i, (fr, _) in enumerate(frames)]
    got = check(exe, tmp_path, items)
    assert {g[0] for g in got} == set(model.ALL_ACTIONS)


def test_stale_action_gives_no_reply_or_that_actions_reply(exe, tmp_path):
    """Every reply action forced on every frame of a world: the build derives
    the lengths again, so each case is length 0 or the model's reply of that
    action -- and the program has refused any access outside frame and reply."""
    seed, n, slot = cases.WORLDS["packed"]
    frames = cases.world(seed, 120)
    v = cases.verdicts_of(frames)
    eng = cases.engine_table()
    items = [(fr, int(v[i]), None, eng, slot, act, 0, (i + act) % 16, (3 * i + act) % 16)
             for i, (fr, _) in enumerate(frames) for act in model.REPLIES + (0, 1, 5, 7, 13, 31, 255)]
    for cut in (0, 13, 14, 15, 17, 18, 33, 34, 41, 42, 53, 54, 61, 62, 101, 102):
        fr = cases.echo6(bytes(60))[:cut]
        items += [(fr, 9, None, eng, 2048, act, 0, cut % 16, 1) for act in model.REPLIES]
    got = check(exe, tmp_path, items)
    assert sum(g[2] != 0 for g in got) > 100 and sum(g[2] == 0 for g in got) > 100
