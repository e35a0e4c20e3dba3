"""CPU tests of the TX neighbours' C ABI (wc_neigh_tab_*, wc_neigh_apply,
wc_tx_resolve, wc_tx_hold_plan, wc_tx_solicit_build): the names are exported
through the header, the library and the Python mirror, the codes and masks
agree, the table sizes, the two pure host calls, and every argument error
returns before a device is touched (there is no GPU here; the pointers are
poisoned)."""
import re
import subprocess
from pathlib import Path

import numpy as np
import pytest

import tx_neigh_cases as cases
import tx_neigh_model as model
import warpcore_amd as wc
from warpcore_amd import _build, _lib

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "warpcore_gpu" / "wc_cksum.h"
OK, EINVAL = 0, -10001
P = 0x100000  # 16-byte aligned, never dereferenced: every call below returns first
CALLS = ("wc_neigh_tab_init", "wc_neigh_apply", "wc_neigh_tab_lookup", "wc_neigh_tab_stats",
         "wc_tx_resolve", "wc_tx_hold_plan", "wc_tx_solicit_build")
SIZES = ("wc_neigh_tab_bytes", "wc_neigh_apply_scratch", "wc_tx_resolve_scratch")
NEW = ("wc_k_txneigh.hip", "wc_rt_txneigh.cpp", "wc_tx_neigh.h")


def test_names_are_exported():
    syms = subprocess.run(["nm", "-D", "--defined-only", str(_build.build_lib())], check=True,
                          capture_output=True, text=True).stdout
    text = HEADER.read_text()
    for name in CALLS + SIZES:
        assert f" T {name}\n" in syms
        assert name in _lib.SIGNATURES
        assert re.search(rf"\b(int|uint64_t) {name}\(", text)
    for name in ("neigh_tab_bytes", "neigh_tab_init", "neigh_apply", "neigh_tab_lookup",
                 "neigh_tab_stats", "tx_resolve", "tx_hold_plan", "tx_solicit_build", "NR_NAMES",
                 "TH_NAMES", "NR_MASK_SOLICIT", "NR_MASK_MISS", "TH_MASK_HELD"):
        assert name in wc.__all__ and hasattr(wc, name)


def test_codes_and_masks_agree():
    text = HEADER.read_text()
    for name, code in (("READY", 0), ("BAD_AF", 4), ("MISS", 8), ("MISS_DUP", 9)):
        assert re.search(rf"\bWC_NR_{name} = {code}\b", text)
        assert getattr(wc, f"NR_{name}") == code == getattr(model, name)
        assert f"NR_{name}" in wc.__all__ and code in wc.NR_NAMES
    for name, code in (("READY", 0), ("MALFORMED", 4), ("HELD", 8)):
        assert re.search(rf"\bWC_TH_{name} = {code}\b", text)
        assert getattr(wc, f"TH_{name}") == code == getattr(model, f"TH_{name}")
        assert f"TH_{name}" in wc.__all__ and code in wc.TH_NAMES
    assert "#define WC_NR_MASK_SOLICIT (0x100u)" in text and "#define WC_NR_MASK_MISS    (0x300u)" in text
    assert "#define WC_TH_MASK_HELD (0x100u)" in text
    assert wc.NR_MASK_SOLICIT == model.MASK_SOLICIT == 1 << wc.NR_MISS
    assert wc.NR_MASK_MISS == model.MASK_MISS == (1 << wc.NR_MISS) | (1 << wc.NR_MISS_DUP)
    assert wc.TH_MASK_HELD == model.MASK_HELD == 1 << wc.TH_HELD
    assert "#define WC_NEIGH_TAB_MIN_CAP 64u" in text and "#define WC_NEIGH_TAB_MAX_CAP (1u << 20)" in text
    assert (wc.NEIGH_TAB_MIN_CAP, wc.NEIGH_TAB_MAX_CAP) == (64, 1 << 20)
    assert wc.TX_DST == model.DST and wc.TX_SOCK == model.SOCK and wc.TX_DESC == model.DESC
    assert wc.NEIGH_UPDATE == model.UPDATE


def test_new_sources_are_built_and_read_no_environment():
    names = {p.name for p in _build.HIP_SOURCES}
    assert {"wc_k_txneigh.hip", "wc_rt_txneigh.cpp"} <= names
    assert "wc_tx_neigh.h" in {p.name for p in _build.HIP_DEPS}
    for name in NEW:
        assert "getenv" not in (ROOT / "warpcore_amd" / "csrc" / name).read_text()


def test_enum_sizes(tmp_path):
    src = tmp_path / "sizes.c"
    src.write_text('#include <stdio.h>\n#include "warpcore_gpu/wc_cksum.h"\n'
                   "int main(void) { printf(\"%d %d %d %d %u %u\\n\", WC_NR_MISS, WC_NR_MISS_DUP, "
                   "WC_TH_HELD, WC_TH_MALFORMED, WC_NEIGH_TAB_MIN_CAP, WC_NEIGH_TAB_MAX_CAP); "
                   "return 0; }\n")
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c11", f"-I{ROOT / 'include'}", str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()
    assert [int(x) for x in out] == [8, 9, 8, 4, 64, 1 << 20]


def test_table_bytes_for_good_and_bad_caps():
    lib = _lib.load()
    for k in range(6, 21):
        assert lib.wc_neigh_tab_bytes(1 << k) == 64 + 32 * (1 << k) == wc.neigh_tab_bytes(1 << k)
    for cap in (0, 1, 32, 63, 65, 96, 127, (1 << 20) + 1, 1 << 21, 0xFFFFFFFF, (1 << 20) - 1):
        assert lib.wc_neigh_tab_bytes(cap) == 0
        with pytest.raises(ValueError):
            wc.neigh_tab_bytes(cap)
        assert lib.wc_neigh_tab_init(P, cap, None) == EINVAL
    assert lib.wc_neigh_apply_scratch(0) == 0 and lib.wc_neigh_apply_scratch(300) == 1200
    assert lib.wc_tx_resolve_scratch(0) == 0 and lib.wc_tx_resolve_scratch(65537) == 0
    prev = 0
    for n in (1, 2, 31, 32, 33, 64, 65, 4097, 65536):
        b = lib.wc_tx_resolve_scratch(n)
        assert b >= 4 * 2 * 2 * n and b >= prev and b >= lib.wc_rx_select_scratch(n)
        prev = b


def test_init_and_apply_argument_errors_need_no_gpu():
    lib = _lib.load()
    assert lib.wc_neigh_tab_init(None, 64, None) == EINVAL
    for t in (P + 1, P + 4, P + 8, P + 15):
        assert lib.wc_neigh_tab_init(t, 64, None) == EINVAL

    def apply(tab=P, upd=P, cnt=P, m=8, dropped=P, scratch=P):
        return lib.wc_neigh_apply(tab, upd, cnt, m, dropped, scratch, None)

    assert lib.wc_neigh_apply(None, None, None, 0, None, None, None) == OK  # m = 0: no pointer
    for missing in ("tab", "upd", "cnt", "scratch"):
        assert apply(**{missing: None}) == EINVAL, missing
    for t in (P + 1, P + 4, P + 8):
        assert apply(tab=t) == EINVAL
    for x in (P + 1, P + 2, P + 3):
        assert apply(upd=x) == EINVAL and apply(scratch=x) == EINVAL
    assert apply(m=(1 << 31) + 1) == EINVAL


def test_resolve_argument_errors_need_no_gpu():
    lib = _lib.load()

    def resolve(tab=P, dsts=P, af=P, ndst=8, state=P, lst=None, cnt=None, scratch=P):
        return lib.wc_tx_resolve(tab, dsts, af, ndst, state, lst, cnt, scratch, None)

    assert lib.wc_tx_resolve(None, None, None, 0, None, None, None, None, None) == OK
    for n in (0, 8, 65537):
        assert resolve(ndst=n, lst=P) == EINVAL and resolve(ndst=n, cnt=P) == EINVAL
    assert resolve(ndst=65537) == EINVAL and resolve(ndst=65537, lst=P, cnt=P) == EINVAL
    for missing in ("tab", "dsts", "af", "state", "scratch"):
        assert resolve(**{missing: None}) == EINVAL, missing
        assert resolve(lst=P, cnt=P, **{missing: None}) == EINVAL, missing
    for t in (P + 1, P + 4, P + 8):
        assert resolve(tab=t) == EINVAL
    for x in (P + 1, P + 2, P + 3):
        assert resolve(dsts=x) == EINVAL and resolve(scratch=x) == EINVAL


def test_hold_plan_argument_errors_need_no_gpu():
    lib = _lib.load()

    def hold(desc=P, n=8, socks=P, ns=4, state=P, af=P, ndst=8, out=P, lst=None, cnt=None,
             scratch=None):
        return lib.wc_tx_hold_plan(desc, n, socks, ns, state, af, ndst, out, lst, cnt, scratch, None)

    assert lib.wc_tx_hold_plan(None, 0, None, 0, None, None, 0, None, None, None, None, None) == OK
    for n in (0, 8):
        assert hold(n=n, lst=P, scratch=P) == EINVAL and hold(n=n, cnt=P, scratch=P) == EINVAL
    assert hold(n=(1 << 32) + 1) == EINVAL and hold(ns=257) == EINVAL and hold(ndst=65537) == EINVAL
    for missing in ("desc", "socks", "state", "af", "out"):
        assert hold(**{missing: None}) == EINVAL, missing
    for x in (P + 1, P + 2, P + 4):
        assert hold(desc=x) == EINVAL
    for x in (P + 1, P + 2, P + 3):
        assert hold(socks=x) == EINVAL
        assert hold(lst=P, cnt=P, scratch=x) == EINVAL
    assert hold(lst=P, cnt=P, scratch=None) == EINVAL


def test_solicit_build_argument_errors_need_no_gpu():
    lib = _lib.load()

    def build(dsts=P, af=P, ndst=8, lst=P, cnt=P, eng=P, out=P, ooff=P, m=4, slot=2048, olen=P,
              built=P):
        return lib.wc_tx_solicit_build(dsts, af, ndst, lst, cnt, eng, out, ooff, m, slot, olen, built,
                                       None)

    assert build(ndst=65537) == EINVAL and build(slot=65536) == EINVAL
    assert build(built=None) == EINVAL and build(built=None, m=0) == EINVAL
    for missing in ("dsts", "af", "lst", "cnt", "eng", "out", "ooff", "olen"):
        assert build(**{missing: None}) == EINVAL, missing
    assert build(ndst=0, olen=None) == EINVAL
    for x in (P + 1, P + 2, P + 3):
        assert build(eng=x) == EINVAL and build(dsts=x) == EINVAL


def test_host_lookup_and_stats_over_a_host_copy():
    lib = _lib.load()
    tab = np.zeros(wc.neigh_tab_bytes(64) // 4, np.uint32)
    mac = np.zeros(8, np.uint8)
    addr = np.zeros(16, np.uint8)
    # bytes init did not write; NULLs; a bad family; a misaligned copy
    assert lib.wc_neigh_tab_lookup(tab.ctypes.data, 4, addr.ctypes.data, mac.ctypes.data) == EINVAL
    assert lib.wc_neigh_tab_stats(tab.ctypes.data, None, None) == EINVAL
    with pytest.raises(ValueError):
        wc.neigh_tab_stats(tab)
    tab[0], tab[1] = 0x4254434E, 64  # an empty table, as wc_neigh_tab_init leaves it
    assert wc.neigh_tab_stats(tab) == (64, 0)
    assert lib.wc_neigh_tab_lookup(None, 4, addr.ctypes.data, mac.ctypes.data) == EINVAL
    assert lib.wc_neigh_tab_lookup(tab.ctypes.data, 4, None, mac.ctypes.data) == EINVAL
    assert lib.wc_neigh_tab_lookup(tab.ctypes.data, 4, addr.ctypes.data, None) == EINVAL
    assert lib.wc_neigh_tab_lookup(tab.ctypes.data + 1, 4, addr.ctypes.data, mac.ctypes.data) == EINVAL
    for af in (0, 5, 7, 255):
        assert lib.wc_neigh_tab_lookup(tab.ctypes.data, af, addr.ctypes.data, mac.ctypes.data) == EINVAL
        with pytest.raises(ValueError):
            wc.neigh_tab_lookup(tab, af, bytes(16))
    for af, a in cases.keys(20) + cases.lookalikes():
        assert wc.neigh_tab_lookup(tab, af, a) is None
    tab[1] = 96  # a cap that is no power of two
    with pytest.raises(ValueError):
        wc.neigh_tab_lookup(tab, 4, bytes(4))


def test_python_wrappers_check_before_the_library():
    import torch
    cpu = torch.zeros(64 + 32 * 64, dtype=torch.uint8)
    with pytest.raises(ValueError):
        wc.neigh_tab_init(64)
    with pytest.raises(ValueError):
        wc.neigh_tab_init(64, tab=cpu)
    with pytest.raises(ValueError):
        wc.neigh_tab_init(65, device="cuda")
    with pytest.raises(ValueError):
        wc.neigh_apply(cpu, cpu, cpu)
    with pytest.raises(ValueError):
        wc.tx_resolve(cpu, cpu, cpu)
    with pytest.raises(ValueError):
        wc.tx_hold_plan(cpu, cpu, cpu, cpu)
    with pytest.raises(ValueError):
        wc.tx_solicit_build(cpu, cpu, cpu, cpu, cpu, cpu, cpu, 86)
