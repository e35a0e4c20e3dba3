"""CPU test of the lines the RX neighbour kernels compile
(warpcore_amd/csrc/wc_rx_neigh.h), compiled for the host alone
(tests/c/rx_neigh_words.cpp, with -fsanitize=address,undefined, run directly):
chain codes, update records and reply bytes against tests/rx_neigh_model.py
over the grid, the four known answers and a world, at all 16 byte phases of
source and destination.  The program itself refuses a load that does not
overlap the frame and a store that is misaligned or leaves the reply."""
import struct
import subprocess

import pytest

import cprog
import rx_neigh_cases as cases
import rx_neigh_model as model
import rx_reply_cases as rc

REGION = 256
REC = 8 + 24 + REGION
OWN = 0xFFFFFFFF


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return cprog.build_words("rx_neigh_words", tmp_path_factory.mktemp("rxn"))


def run(exe, tmp_path, items):
    """items: (frame, action, engine, code or OWN, slot_bytes, source phase,
    destination phase) -> [(code, out_len, record bytes, region bytes)]."""
    blob = bytearray()
    for fr, act, eng, code, slot, sp, dp in items:
        blob += eng.tobytes()
        blob += struct.pack("<6I", act, code, slot, sp, dp, len(fr))
        blob += fr
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(bytes(blob))
    r = subprocess.run([str(exe), str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw = dst.read_bytes()
    assert len(raw) == len(items) * REC
    return [struct.unpack("<2I", raw[i:i + 8]) + (raw[i + 8:i + 32], raw[i + 32:i + REC])
            for i in range(0, len(raw), REC)]


def want_of(fr, act, eng, code, slot, dp):
    c = model.plan(fr, act, eng)
    use = c if code == OWN else code
    reply = model.build(fr, use, eng)
    if reply is not None and len(reply) > slot:
        reply = None
    region = bytearray(b"\xa5" * REGION)
    if reply is not None:
        region[16 + dp:16 + dp + len(reply)] = reply
    return c, len(reply) if reply is not None else 0, model.record_bytes(fr, use), bytes(region)


def check(exe, tmp_path, items):
    got = run(exe, tmp_path, items)
    for i, (g, it) in enumerate(zip(got, items)):
        fr, act, eng, code, slot, sp, dp = it
        assert g == want_of(fr, act, eng, code, slot, dp), f"case {i}: phases {sp}/{dp}, code {code}"
    return got


def test_grid_every_phase(exe, tmp_path):
    grid = cases.grid()
    items = [(fr, act, eng, OWN, 2048, sp, (5 * sp + j) % 16)
             for sp in range(16) for j, (_, fr, act, eng, _) in enumerate(grid)]
    got = check(exe, tmp_path, items)
    for g, (name, _, _, _, code) in zip(got, grid * 16):
        assert g[0] == code, name


def test_known_answers_every_source_and_destination_phase(exe, tmp_path):
    eng = rc.engine_table()
    nsol, arp = bytes.fromhex(cases.NSOL_HEX), bytes.fromhex(cases.ARP_HEX)
    items = [(fr, model.HOST, eng, OWN, slot, sp, dp) for sp in range(16) for dp in range(16)
             for fr, slot in ((nsol, 86), (arp, 42))]
    got = check(exe, tmp_path, items)
    for (code, ln, rec, region), (fr, _, _, _, _, _, dp) in zip(got, items):
        want = cases.NADV_HEX if fr is nsol else cases.IS_AT_HEX
        assert region[16 + dp:16 + dp + ln].hex() == want
    assert got[0][2] == bytes((6, model.NADV)) + rc.PEER_MAC + rc.PEER6
    assert got[1][2] == bytes((4, model.ARP_IS_AT)) + rc.PEER_MAC + rc.PEER4 + bytes(12)


def test_slot_bytes_around_both_lengths(exe, tmp_path):
    eng = rc.engine_table()
    nsol, arp = bytes.fromhex(cases.NSOL_HEX), bytes.fromhex(cases.ARP_HEX)
    items = [(fr, model.HOST, eng, OWN, slot, 3, dp) for dp in range(4)
             for fr, slots in ((nsol, (0, 42, 85, 86, 87)), (arp, (0, 41, 42, 43))) for slot in slots]
    got = check(exe, tmp_path, items)
    assert [g[1] for g in got[:9]] == [0, 0, 0, 86, 86, 0, 0, 42, 42]


def test_world_and_stale_codes(exe, tmp_path):
    """A world with the plan's own codes, then every code forced on every
    frame: the record and the build derive the bounds again, so each case is
    an empty record / length 0 or the model's -- and the program has refused
    any access outside frame and reply."""
    seed, n = cases.WORLDS["slots"]
    frames = cases.world(seed, n)
    eng = rc.engine_table()
    act = cases.actions_of(frames, eng)
    items = [(fr, int(act[i]), eng, OWN, 2048, i % 16, (i // 16) % 16)
             for i, (fr, _, _) in enumerate(frames)]
    got = check(exe, tmp_path, items)
    assert {g[0] for g in got} == set(model.ALL_ACTIONS)
    stale = [(fr, int(act[i]), eng, code, 86, (i + code) % 16, (3 * i + code) % 16)
             for i, (fr, _, _) in enumerate(frames[:150])
             for code in model.UPDATES + (0, 1, 4, 7, 12, 31, 255)]
    got = check(exe, tmp_path, stale)
    assert sum(g[1] != 0 for g in got) > 100 and sum(g[1] == 0 for g in got) > 100
    assert sum(any(g[2]) for g in got) > 100 and sum(not any(g[2]) for g in got) > 100
