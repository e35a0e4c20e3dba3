"""CPU tests of the RX drain's C ABI (wc_rx_drain_scratch, wc_rx_drain): the
names are exported through the header, the library and the Python mirror, the
scratch size is 0 at n = 0, never decreases and covers both of the chain's, the
output struct is fifteen pointers, and every argument error returns before a
device is touched (there is no GPU here; the pointers are poisoned)."""
import ctypes
import re
import subprocess
from pathlib import Path

import pytest

import warpcore_amd as wc
from warpcore_amd import _build, _lib
from warpcore_amd.cksum import _DrainOut

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "warpcore_gpu" / "wc_cksum.h"
OK, EINVAL = 0, -10001
P = 0x100000  # 16-byte aligned, never dereferenced: every call below returns first
MEMBERS = [name for name, _ in _DrainOut._fields_]


def test_drain_names_are_exported():
    syms = subprocess.run(["nm", "-D", "--defined-only", str(_build.build_lib())], check=True,
                          capture_output=True, text=True).stdout
    text = HEADER.read_text()
    assert " T wc_rx_drain\n" in syms and " T wc_rx_drain_scratch\n" in syms
    assert re.search(r"\bint wc_rx_drain\(", text) and re.search(r"\buint64_t wc_rx_drain_scratch\(", text)
    assert "#define WC_RX_DRAIN_SMALL 4096u" in text and wc.RX_DRAIN_SMALL == 4096
    for name in ("wc_rx_drain", "wc_rx_drain_scratch"):
        assert name in _lib.SIGNATURES
    for name in ("rx_drain", "rx_drain_scratch", "RxDrain", "RX_DRAIN_SMALL"):
        assert name in wc.__all__ and hasattr(wc, name)
    assert len(wc.RxDrain._fields) == 15


def test_new_sources_are_built_and_read_no_environment():
    names = {p.name for p in _build.HIP_SOURCES}
    assert {"wc_k_rxdrain.hip", "wc_rt_rxdrain.cpp"} <= names
    assert "wc_rx_demux.h" in {p.name for p in _build.HIP_DEPS}
    for name in ("wc_k_rxdrain.hip", "wc_rt_rxdrain.cpp", "wc_rx_demux.h"):
        assert "getenv" not in (ROOT / "warpcore_amd" / "csrc" / name).read_text()


def test_scratch_size():
    lib = _lib.load()
    assert lib.wc_rx_drain_scratch(0) == 0 == wc.rx_drain_scratch(0)
    ns = sorted(set(list(range(0, 70)) + [4095, 4096, 4097, 8191, 8192, 8193, 65535, 65536, 65537]
                    + [(1 << k) + d for k in range(17, 33) for d in (-1, 0, 1)]))
    sizes = [lib.wc_rx_drain_scratch(n) for n in ns]
    assert all(a <= b for a, b in zip(sizes, sizes[1:])), "never decreasing in n"
    assert all(s > 0 for n, s in zip(ns, sizes) if n > 0)
    for n, s in zip(ns, sizes):
        if n > 4096:  # the fallback's calls share it
            assert s >= lib.wc_rx_select_scratch(n) and s >= lib.wc_rx_demux_scratch(n), n


def test_out_struct_is_fifteen_pointers(tmp_path):
    src = tmp_path / "sizes.c"
    offs = ", ".join(f"offsetof(struct wc_rx_drain_out, {m})" for m in MEMBERS)
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "warpcore_gpu/wc_cksum.h"\n'
                   "int main(void) { size_t v[] = {sizeof(struct wc_rx_drain_out), sizeof(void *), "
                   f"{offs}}};\n"
                   "for (unsigned i = 0; i < sizeof v / sizeof *v; ++i) printf(\"%zu \", v[i]); "
                   "return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)],
                   check=True)
    out = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True,
                                          text=True).stdout.split()]
    ptr = out[1]
    assert out[0] == 15 * ptr == ctypes.sizeof(_DrainOut)
    assert out[2:] == [k * ptr for k in range(15)] == [getattr(_DrainOut, m).offset for m in MEMBERS]


def drain(lib, base=P, off=P, flen=P, n=8, tab=P, ns=3, eng=P, slot=2048, out=True, scratch=P, **members):
    o = _DrainOut(*[members.get(m, P) for m in MEMBERS])
    return lib.wc_rx_drain(base, off, flen, n, tab, ns, eng, slot,
                           ctypes.byref(o) if out else None, scratch, None)


def test_argument_errors_need_no_gpu():
    lib = _lib.load()
    for n in (0, 8, 5000):
        assert drain(lib, n=n, out=False) == EINVAL  # a NULL out, for every n
        assert drain(lib, n=n, ns=255) == EINVAL
        for m in ("start", "rcount", "nrcount", "ucount"):
            assert drain(lib, n=n, **{m: None}) == EINVAL, (n, m)
    assert drain(lib, n=(1 << 32) + 1) == EINVAL
    for n in (8, 4096, 4097):
        assert drain(lib, n=n, slot=65536) == EINVAL
        for missing in ("base", "off", "flen", "tab", "eng", "scratch"):
            assert drain(lib, n=n, **{missing: None}) == EINVAL, (n, missing)
        for m in MEMBERS:
            if m != "drops":
                assert drain(lib, n=n, **{m: None}) == EINVAL, (n, m)
        for d in (1, 2, 3):
            assert drain(lib, n=n, eng=P + d) == EINVAL
            assert drain(lib, n=n, tab=P + d) == EINVAL
            assert drain(lib, n=n, scratch=P + d) == EINVAL
        for d in (1, 2, 4, 8):
            assert drain(lib, n=n, rec=P + d) == EINVAL


def test_python_wrapper_checks_before_the_library():
    import torch
    cpu = torch.zeros(64, dtype=torch.uint8)
    with pytest.raises(ValueError):
        wc.rx_drain(cpu, cpu, cpu, cpu, 0, cpu)
    assert wc.rx_drain_scratch(4097) >= max(wc.rx_select_scratch(4097), wc.rx_demux_scratch(4097))
