"""CPU tests of the TX seal's C ABI (wc_tx_seal_ragged / wc_tx_seal_host):
the names are exported through the header, the library and the Python mirror,
the status codes are 0..7, and every argument error returns before a device
is touched (there is no GPU here)."""
import re
from pathlib import Path

import numpy as np

import warpcore_amd as wc
from warpcore_amd import _build, _lib

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "warpcore_gpu" / "wc_cksum.h"
OK, EINVAL = 0, -10001
ZERO_UDP, NO_STORE = 1, 2


def test_tx_names_are_exported():
    import subprocess
    syms = subprocess.run(["nm", "-D", "--defined-only", str(_build.build_lib())], check=True,
                          capture_output=True, text=True).stdout
    for name in ("wc_tx_seal_ragged", "wc_tx_seal_host"):
        assert f" T {name}\n" in syms
        assert name in _lib.SIGNATURES
        assert re.search(rf"\bint {name}\(", HEADER.read_text())
    for name in ("tx_seal_ragged", "tx_seal_host", "TX_ERRORS", "TX_SEALED", "TX_TRUNCATED"):
        assert name in wc.__all__ and hasattr(wc, name)


def test_tx_status_codes_are_0_to_7():
    names = ("SEALED", "SEALED_ZERO_UDP", "IP_ONLY", "NOT_UDP", "NOT_IP", "BAD_VERSION",
             "MALFORMED", "TRUNCATED")
    text = HEADER.read_text()
    for value, name in enumerate(names):
        assert re.search(rf"\bWC_TX_{name} = {value},", text), name
        assert getattr(wc, f"TX_{name}") == value
    assert wc.TX_ERRORS == (wc.TX_BAD_VERSION, wc.TX_MALFORMED, wc.TX_TRUNCATED)
    assert "#define WC_TX_IS_ERROR(s) ((s) >= WC_TX_BAD_VERSION)" in text
    assert "#define WC_TX_ZERO_UDP_CKSUM 1u" in text and "#define WC_TX_NO_STORE 2u" in text
    assert len(wc.TX_NAMES) == 8


def test_tx_seal_ragged_argument_errors_need_no_gpu():
    lib = _lib.load()
    p = 0x100000  # never dereferenced: every call below returns first
    assert lib.wc_tx_seal_ragged(None, None, None, 0, 0, None, None, None, None, None) == OK
    for missing in range(4):  # base, offsets, lengths, status
        a = [p, p, p, p]
        a[missing] = None
        assert lib.wc_tx_seal_ragged(a[0], a[1], a[2], 8, 0, a[3], p, p, p, None) == EINVAL
    for flags in (4, 8, 0x80000000, ZERO_UDP | 4):  # unknown flag bits
        assert lib.wc_tx_seal_ragged(p, p, p, 8, flags, p, p, p, None, None) == EINVAL
    # compute only: both value arrays are required
    assert lib.wc_tx_seal_ragged(p, p, p, 8, NO_STORE, p, None, p, None, None) == EINVAL
    assert lib.wc_tx_seal_ragged(p, p, p, 8, NO_STORE, p, p, None, None, None) == EINVAL
    assert lib.wc_tx_seal_ragged(p, p, p, 8, NO_STORE | ZERO_UDP, p, None, None, None,
                                 None) == EINVAL


def test_tx_seal_host_argument_errors_need_no_gpu():
    lib = _lib.load()
    buf = np.zeros(100, dtype=np.uint8)
    off = np.array([40], dtype=np.uint64)
    ln = np.array([60], dtype=np.uint16)
    st = np.zeros(1, dtype=np.uint8)
    b, o, n_, s = (a.ctypes.data for a in (buf, off, ln, st))
    assert lib.wc_tx_seal_host(None, 0, None, None, 0, 0, None, None) == OK
    assert lib.wc_tx_seal_host(None, 100, o, n_, 1, 0, s, None) == EINVAL
    assert lib.wc_tx_seal_host(b, 100, None, n_, 1, 0, s, None) == EINVAL
    assert lib.wc_tx_seal_host(b, 100, o, None, 1, 0, s, None) == EINVAL
    assert lib.wc_tx_seal_host(b, 100, o, n_, 1, 0, None, None) == EINVAL
    assert lib.wc_tx_seal_host(b, 100, o, n_, 1, NO_STORE, s, None) == EINVAL
    assert lib.wc_tx_seal_host(b, 100, o, n_, 1, 4, s, None) == EINVAL
    off[0] = 41  # 60 bytes from 41: past the 100-byte region
    assert lib.wc_tx_seal_host(b, 100, o, n_, 1, 0, s, None) == EINVAL
    off[0] = 101
    assert lib.wc_tx_seal_host(b, 100, o, n_, 1, ZERO_UDP, s, None) == EINVAL
    assert not buf.any()
