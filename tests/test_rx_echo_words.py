"""CPU test of the lines the RX echo kernel compiles
(warpcore_amd/csrc/wc_rx_echo.h), compiled for the host alone under ASan /
UBSan (tests/c/rx_echo_words.cpp): every entry's socket and list position, the
echo count and the grid size against tests/rx_echo_model.py over start arrays
with stale entries, and the payload copy at all 256 phase pairs on a checked
memory."""
import struct
import subprocess

import numpy as np
import pytest

import cprog
import rx_echo_cases as cases
import rx_echo_model as model

RUNS = (0, 1, 63, 64, 65, 4096)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return cprog.build_words("rx_echo_words", tmp_path_factory.mktemp("rxe"))


def starts_of(lens, tail: int = 0) -> np.ndarray:
    """start[256] of runs of these lengths, `tail` unbound frames behind them."""
    start = np.zeros(256, np.uint64)
    start[1:len(lens) + 1] = np.cumsum(lens)
    start[len(lens) + 1:255] = start[len(lens)]
    start[255] = start[254] + np.uint64(tail)
    return start


def worlds():
    """[(n, ns, m, start, map)]: ns in {0, 1, 2, 253, 254}, run lengths from
    RUNS (a run of 4096 now and then), the four maps, and stale starts: a
    decreasing pair, an entry above n, an n below the list's total, n = 0."""
    rng = np.random.default_rng(8)
    out = []
    for ns in (0, 1, 2, 253, 254):
        for kind in ("all", "none", "alternating", "single"):
            for rep in range(3):
                p = (.2, .2, .15, .15, .15, .15) if ns <= 2 else (.3, .3, .12, .12, .12, .04)
                lens = np.array(RUNS)[np.searchsorted(np.cumsum(p)[:-1], rng.random(ns), "right")]
                start = starts_of(lens, int(rng.integers(0, 50)))
                n = int(start[255]) + int(rng.integers(0, 3))
                emap = cases.echo_map(ns, kind, one=int(rng.integers(0, max(ns, 1))))
                m = int(rng.choice((0, 1, 63, 64, 65, 4096, 65536)))
                out.append((n, ns, m, start, emap))
                if ns >= 2 and rep == 0:
                    stale = start.copy()                    # decreasing: run s - 1 and the runs
                    s = int(rng.integers(1, ns))            # whose end lies above n are empty
                    stale[s] = stale[s] // np.uint64(2)
                    out.append((n, ns, m, stale, emap))
                    stale = start.copy()
                    stale[int(rng.integers(1, ns + 1))] = n + 1 + int(rng.integers(0, 1 << 40))
                    out.append((n, ns, m, stale, emap))
                    out.append((int(start[ns // 2]), ns, m, start, emap))   # a smaller ring
                    out.append((0, ns, m, start, emap))
    return out


def test_every_entry_maps_as_the_model_says(exe, tmp_path):
    ws = worlds()
    blob = bytearray()
    for n, ns, m, start, emap in ws:
        pad = np.zeros(256, np.uint16)
        pad[:ns] = emap
        blob += struct.pack("<QII", n, ns, m) + start.tobytes() + pad.tobytes()
    src, dst = tmp_path / "in.bin", tmp_path / "out.bin"
    src.write_bytes(bytes(blob))
    r = subprocess.run([str(exe), "map", str(src), str(dst)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    raw, at, some = dst.read_bytes(), 0, 0
    for n, ns, m, start, emap in ws:
        E, grid, _ = struct.unpack_from("<QII", raw, at)
        at += 16
        want = model.order(start, emap, n) if n and ns else []
        assert E == len(want), (n, ns)
        assert grid == max(1, -(-m // 64)), m
        got = np.frombuffer(raw, np.dtype([("s", "<u4"), ("z", "<u4"), ("at", "<u8")]), E, at)
        at += 16 * E
        if E:
            w = np.array(want, np.uint64)
            assert (got["s"] == w[:, 0]).all() and (got["at"] == w[:, 1]).all(), (n, ns)
            some += 1
    assert at == len(raw) and some > 40


def test_copy_every_phase_pair_on_checked_memory(exe):
    r = subprocess.run([str(exe), "copy"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert int(r.stdout) == 256 * 51
