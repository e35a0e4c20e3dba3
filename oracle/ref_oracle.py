"""TEST INFRASTRUCTURE ONLY -- ctypes binding of the reference's own checksum
object, oracle/_ref/libwc_ref.so: lib/src/in_cksum.c of the reference compiled
unchanged (oracle/Makefile, target `ref`), its two functions renamed wcref_*.

The restatements (wc_oracle.c, py_oracle.py) stay the fast parity checker and
the CPU baseline; this module is what pins them -- and, through the recorded
results in tests/golden/ref_vectors.npz, the kernels -- to the code they
restate.  Where the reference tree exists the object is built on demand;
elsewhere (a GPU host) the copy that came with the tree is loaded.

payload_cksum(buf, len) with len below the IP header length is not defined in
the reference (a ~4 GiB read): the payload entry points raise ValueError for
such a call and never pass it on.
"""
from __future__ import annotations

import ctypes
import threading

import numpy as np

_lock = threading.Lock()
_lib = None

KIND_IP, KIND_PAYLOAD = 0, 1


def path():
    """The object's path (built first where the reference tree exists), or
    None where there is neither an object nor a tree to build it from."""
    from warpcore_amd import _build  # build recipe only (no product code)
    return _build.build_ref()


def available() -> bool:
    return path() is not None


def load() -> ctypes.CDLL:
    global _lib
    with _lock:
        if _lib is None:
            p = path()
            if p is None:
                raise RuntimeError("no oracle/_ref/libwc_ref.so and no reference tree "
                                   "(WC_REFERENCE_DIR) to build it from")
            lib = ctypes.CDLL(str(p))
            u16, u64, i, vp = ctypes.c_uint16, ctypes.c_uint64, ctypes.c_int, ctypes.c_void_p
            sig = {
                "wcref_ip_cksum": (u16, [vp, u16]),
                "wcref_payload_cksum_checked": (i, [vp, u16, ctypes.POINTER(u16)]),
                "wcref_cksum_ragged": (ctypes.c_int64, [vp, vp, vp, u64, vp, i]),
            }
            for name, (res, args) in sig.items():
                fn = getattr(lib, name)
                fn.restype = res
                fn.argtypes = args
            _lib = lib
    return _lib


def _u8(buf) -> np.ndarray:
    if not isinstance(buf, np.ndarray):
        buf = np.frombuffer(bytes(buf), dtype=np.uint8)
    return np.ascontiguousarray(buf).reshape(-1).view(np.uint8)


def hdr_len(first_byte):
    """The header length payload_cksum takes from a packet's first byte:
    4 * IHL where the high nibble is 4, 40 otherwise (scalar or array)."""
    b = np.asarray(first_byte).astype(np.uint32)
    return np.where(b >> 4 == 4, (b & 0x0F) * 4, 40)


def ip_cksum(buf, length=None) -> int:
    a = _u8(buf)
    length = a.size if length is None else int(length)
    if not 0 <= length <= 0xFFFF or length > a.size:
        raise ValueError("len outside the buffer or past 65535")
    if a.size == 0:
        a = np.zeros(1, np.uint8)
    return int(load().wcref_ip_cksum(a.ctypes.data, length))


def payload_cksum(buf, length=None) -> int:
    a = _u8(buf)
    length = a.size if length is None else int(length)
    if not 0 <= length <= 0xFFFF:
        raise ValueError("len past 65535")
    if a.size < 1:
        raise ValueError("empty buffer")
    hl = int(hdr_len(a[0]))
    if length < hl:
        raise ValueError(f"len {length} < IP header length {hl}: the reference reads ~4 GiB")
    # the header fields are read whatever len is: IPv4 up to byte 19, IPv6 up to 39
    if a.size < max(length, 20 if a[0] >> 4 == 4 else 40):
        raise ValueError("buffer shorter than what payload_cksum reads")
    out = ctypes.c_uint16()
    if load().wcref_payload_cksum_checked(a.ctypes.data, length, ctypes.byref(out)) != 0:
        raise ValueError("len < IP header length")
    return int(out.value)


def cksum_ragged(buf, off, lens, kind: int = 0) -> np.ndarray:
    """The reference's checksums of buf[off[i] : off[i] + lens[i]]."""
    a = _u8(buf)
    off = np.ascontiguousarray(off, dtype=np.uint64)
    lens = np.ascontiguousarray(lens, dtype=np.uint16)
    if off.shape != lens.shape or off.ndim != 1:
        raise ValueError("off and lens must be 1-D arrays of one size")
    if kind not in (KIND_IP, KIND_PAYLOAD):
        raise ValueError("kind must be 0 (ip_cksum) or 1 (payload_cksum)")
    out = np.empty(off.size, dtype=np.uint16)
    if off.size == 0:
        return out
    span = lens.astype(np.int64)
    if kind == KIND_PAYLOAD:
        if int(off.max()) >= a.size:
            raise ValueError("a packet starts past the buffer")
        first = a[off.astype(np.int64)]
        hl = hdr_len(first)
        bad = np.flatnonzero(span < hl)
        if bad.size:
            raise ValueError(f"{bad.size} packets with len < IP header length (first: index "
                             f"{int(bad[0])}): the reference reads ~4 GiB")
        span = np.maximum(span, np.where(first >> 4 == 4, 20, 40))
    if int((off.astype(np.int64) + span).max()) > a.size:
        raise ValueError("a packet runs past the buffer")
    base = a.ctypes.data if a.size else 0
    r = load().wcref_cksum_ragged(base, off.ctypes.data, lens.ctypes.data, off.size,
                                  out.ctypes.data, kind)
    if r >= 0:
        raise ValueError(f"packet {r}: len < IP header length")
    return out
