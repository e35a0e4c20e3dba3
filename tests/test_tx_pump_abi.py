"""CPU tests of the TX pump's C ABI (wc_tx_pump_scratch, wc_tx_pump): the names
are exported through the header, the library and the Python mirror, the three
constants agree, enum wc_tx_status, WC_TX_IS_ERROR and TX_NAMES are what they
were, the scratch size is monotone and covers the chain's, the output struct is
thirteen pointers, and every argument error returns before a device is touched
(there is no GPU here; the pointers are poisoned and never dereferenced).  The
empty calls (n = 0, ndst = 0, m = 0) write their counts on the device, so they
cannot be made with pointers that are never dereferenced: they are made on real
memory in tests/test_gpu_tx_pump.py."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest

import warpcore_amd as wc
from warpcore_amd import _build, _lib
from warpcore_amd.cksum import _PumpOut

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "warpcore_gpu" / "wc_cksum.h"
OK, EINVAL = 0, -10001
P = 0x100000  # 16-byte aligned, never dereferenced: every call below returns first
MEMBERS = [name for name, _ in _PumpOut._fields_]
OPTIONAL = ("out_ip_hdr", "out_udp", "errors")


def test_pump_names_and_constants():
    syms = subprocess.run(["nm", "-D", "--defined-only", str(_build.build_lib())], check=True,
                          capture_output=True, text=True).stdout
    text = HEADER.read_text()
    assert " T wc_tx_pump\n" in syms and " T wc_tx_pump_scratch\n" in syms
    assert re.search(r"\bint wc_tx_pump\(", text) and re.search(r"\buint64_t wc_tx_pump_scratch\(", text)
    for name, value, mirror in (("WC_TX_PUMP_SMALL", "4096u", wc.TX_PUMP_SMALL),
                                ("WC_TX_PUMP_SMALL_DST", "4096u", wc.TX_PUMP_SMALL_DST),
                                ("WC_TX_PUMP_HELD", "0x80u", wc.TX_PUMP_HELD)):
        m = re.search(rf"#define {name}\s+(\S+)", text)
        assert m and m.group(1) == value and int(value.rstrip("u"), 0) == mirror, name
    for name in ("wc_tx_pump", "wc_tx_pump_scratch"):
        assert name in _lib.SIGNATURES
    for name in ("tx_pump", "tx_pump_scratch", "TxPump", "TX_PUMP_SMALL", "TX_PUMP_SMALL_DST",
                 "TX_PUMP_HELD"):
        assert name in wc.__all__ and hasattr(wc, name)
    assert len(wc.TxPump._fields) == 13 == len(MEMBERS)


def test_status_enum_macro_and_names_are_unchanged():
    text = HEADER.read_text()
    body = re.search(r"enum wc_tx_status \{(.*?)\};", text, re.S).group(1)
    names = re.findall(r"\b(WC_TX_[A-Z0-9_]+) = (\d+),", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [("WC_TX_SEALED", "0"), ("WC_TX_SEALED_ZERO_UDP", "1"), ("WC_TX_IP_ONLY", "2"),
                     ("WC_TX_NOT_UDP", "3"), ("WC_TX_NOT_IP", "4"), ("WC_TX_BAD_VERSION", "5"),
                     ("WC_TX_MALFORMED", "6"), ("WC_TX_TRUNCATED", "7")]
    assert "#define WC_TX_IS_ERROR(s) ((s) >= WC_TX_BAD_VERSION)" in text
    assert wc.TX_NAMES == ("sealed", "sealed_zero_udp", "ip_only", "not_udp", "not_ip", "bad_version",
                           "malformed", "truncated")
    assert wc.TX_PUMP_HELD >= len(wc.TX_NAMES)  # no enum wc_tx_status code
    assert "hold[i]" in text and "WC_TX_IS_ERROR is true" in text  # the caller is told


def test_new_sources_are_built_and_read_no_environment():
    names = {p.name for p in _build.HIP_SOURCES}
    assert {"wc_k_txpump.hip", "wc_rt_txpump.cpp"} <= names
    assert "wc_tx_pump.h" in {p.name for p in _build.HIP_DEPS}
    for name in ("wc_k_txpump.hip", "wc_rt_txpump.cpp", "wc_tx_pump.h"):
        assert "getenv" not in (ROOT / "warpcore_amd" / "csrc" / name).read_text()


def test_scratch_size():
    lib = _lib.load()
    assert lib.wc_tx_pump_scratch(0, 0) == 0 == wc.tx_pump_scratch(0, 0)
    ns = sorted(set(list(range(0, 70)) + [4095, 4096, 4097, 65535, 65536, 65537]
                    + [(1 << k) + d for k in (17, 20, 26, 32) for d in (-1, 0, 1)]))
    ds = sorted(set(list(range(0, 70)) + [255, 256, 257, 4095, 4096, 4097, 32768, 65535, 65536]))
    grid = [[lib.wc_tx_pump_scratch(n, d) for d in ds] for n in ns]
    for i, n in enumerate(ns):
        for j, d in enumerate(ds):
            s = grid[i][j]
            assert s >= lib.wc_tx_resolve_scratch(d) and s >= lib.wc_rx_select_scratch(n), (n, d)
            assert (s > 0) == (n > 0 or d > 0), (n, d)
            assert i == 0 or grid[i - 1][j] <= s, "never decreasing in n"
            assert j == 0 or grid[i][j - 1] <= s, "never decreasing in ndst"
    for n in (0, 1, 4096, 1 << 20):
        assert lib.wc_tx_pump_scratch(n, 65537) == 0 == lib.wc_tx_pump_scratch(n, 0xFFFFFFFF)


def test_out_struct_is_thirteen_pointers(tmp_path):
    src = tmp_path / "sizes.c"
    offs = ", ".join(f"offsetof(struct wc_tx_pump_out, {m})" for m in MEMBERS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "warpcore_gpu/wc_cksum.h"\n'
                   "int main(void) { size_t v[] = {sizeof(struct wc_tx_pump_out), sizeof(void *), "
                   f"{offs}}};\n"
                   "for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf(\"%zu \", v[i]); "
                   "return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    ptr = out[1]
    assert out[0] == 13 * ptr == ctypes.sizeof(_PumpOut)
    assert out[2:] == [k * ptr for k in range(13)] == [getattr(_PumpOut, m).offset for m in MEMBERS]


def pump(lib, tab=P, dsts=P, af=P, ndst=8, desc=P, n=8, socks=P, ns=4, base=P, off=P, slot=2048,
         flags=0, eng=P, sol=P, sol_off=P, m=4, sol_slot=128, out=True, scratch=P, **members):
    o = _PumpOut(*[members.get(x, P) for x in MEMBERS])
    return lib.wc_tx_pump(tab, dsts, af, ndst, desc, n, socks, ns, base, off, slot, flags, eng, sol,
                          sol_off, m, sol_slot, ctypes.byref(o) if out else None, scratch, None)


SIZES = [(8, 8), (4096, 4096), (4097, 8), (8, 4097)]  # both paths


def test_argument_errors_need_no_gpu():
    lib = _lib.load()
    for n, ndst in SIZES + [(0, 0), (0, 8), (8, 0)]:
        assert pump(lib, n=n, ndst=ndst, out=False) == EINVAL
        for c in ("miss_count", "held_count", "sol_built"):
            assert pump(lib, n=n, ndst=ndst, **{c: None}) == EINVAL, (n, ndst, c)
        assert pump(lib, n=n, ndst=ndst, ns=257) == EINVAL
        assert pump(lib, n=n, ndst=ndst, slot=65536) == EINVAL
        assert pump(lib, n=n, ndst=ndst, sol_slot=65536) == EINVAL
        for flags in (2, 3, 4, 0x80000000):  # WC_TX_NO_STORE and any other bit
            assert pump(lib, n=n, ndst=ndst, flags=flags) == EINVAL
    assert pump(lib, n=(1 << 32) + 1) == EINVAL and pump(lib, ndst=65537) == EINVAL
    for n, ndst in SIZES:
        for missing in ("tab", "dsts", "af", "desc", "socks", "base", "off", "eng", "sol", "sol_off",
                        "scratch"):
            assert pump(lib, n=n, ndst=ndst, **{missing: None}) == EINVAL, (n, ndst, missing)
        for x in MEMBERS:
            if x not in OPTIONAL:
                assert pump(lib, n=n, ndst=ndst, **{x: None}) == EINVAL, (n, ndst, x)
        for d in (1, 2, 3):
            for arg in ("dsts", "socks", "eng", "scratch"):
                assert pump(lib, n=n, ndst=ndst, **{arg: P + d}) == EINVAL, (arg, d)
        for d in (1, 2, 4, 8):
            assert pump(lib, n=n, ndst=ndst, tab=P + d) == EINVAL
        for d in (1, 2, 4):
            assert pump(lib, n=n, ndst=ndst, desc=P + d) == EINVAL
    # the scratch is asked for whenever either side is non-empty
    for n, ndst in ((8, 0), (0, 8), (5000, 0), (0, 5000)):
        assert pump(lib, n=n, ndst=ndst, scratch=None) == EINVAL
        assert pump(lib, n=n, ndst=ndst, scratch=P + 2) == EINVAL
    # m > 0 needs its lengths even without a destination
    assert pump(lib, n=0, ndst=0, sol_len=None) == EINVAL


def test_python_wrapper_checks_before_the_library():
    import torch
    cpu = torch.zeros(64 + 32 * 64, dtype=torch.uint8)
    with pytest.raises(ValueError):
        wc.tx_pump(cpu, cpu, cpu, cpu, cpu, cpu, cpu, 2048, cpu, cpu, cpu, 128)
    assert wc.tx_pump_scratch(4097, 300) >= max(wc.rx_select_scratch(4097), wc.tx_resolve_scratch(300))
