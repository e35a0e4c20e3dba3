"""TEST INFRASTRUCTURE ONLY -- the parity oracle for warpcore's checksum.

Importable only by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline
leg.  It is the checker, never the thing measured or shipped.

* :mod:`oracle.c_oracle` -- ctypes binding of the C restatement
  (wc_oracle.c; -Ofast -march=native, pthreads) used at full sizes and as the
  timed CPU baseline.
* :mod:`oracle.py_oracle` -- an independent pure-Python restatement (loops,
  small cases only) used to cross-check the C restatement.

* :mod:`oracle.ref_oracle` -- ctypes binding of the reference's own
  in_cksum.c, compiled unchanged into oracle/_ref/libwc_ref.so (Makefile
  target ``ref``, ref_driver.c) where the reference tree exists: what the two
  restatements are pinned to (tests/test_reference.py) and what
  tests/golden/ref_vectors.npz was recorded from.

Reference restated: /root/reference/lib/src/in_cksum.c:74-167.
Parity status: see wc_oracle.h and DESIGN.md section 3 (both checksum
functions bit-exact against the reference's object over the domain listed
there; the RX and TX decision chains stay restatements; also the known answers
in tests/golden/kat.json and the Linux-kernel-computed checksums in
tests/golden/linux_vectors.npz).
"""
