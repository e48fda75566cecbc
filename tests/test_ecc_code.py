"""The SEC-DED code of the coded threshold memories (csrc/ecc.h), host side (no GPU): bnn_mi355x_ecc_encode /
bnn_mi355x_ecc_decode against the definition's vectors, its guarantees (every single error restored, no double
miscorrected), the plain-Python restatement (tests/ecc_ref.py), and the linearity the kernel relies on: status and
corrected bit depend on the error pattern alone.  All comparisons are exact."""
import ctypes as C
import itertools

import numpy as np

import ecc_ref as er
import gpu_lib as gl

WORDS = [0x0000, 0xFFFF, 0x0001, 0x8000, 0x1234, 0x7FFF, 0xFF80, 0x0080, 0xAAAA, 0x5555] + \
    np.random.default_rng(18).integers(0, 1 << 16, 54).tolist()


def lib_decode(L, d, c):
    out = C.c_uint(0)
    status = L.bnn_mi355x_ecc_decode(d, c, C.byref(out))
    return status, out.value


def flips(positions):
    """error bits 0 ... 15: data; 16 ... 21: check -> (data mask, check mask)"""
    dm = sum(1 << p for p in positions if p < 16)
    cm = sum(1 << (p - 16) for p in positions if p >= 16)
    return dm, cm


def test_vectors():
    L = gl.load("cnvW1A1")
    for d, c in ((0x0001, 0x23), (0x8000, 0x15), (0xFFFF, 0x1E), (0x1234, 0x19), (0x0000, 0x00)):
        assert L.bnn_mi355x_ecc_encode(d) == c and er.encode(d) == c, hex(d)
        assert lib_decode(L, d, c) == (0, d)
    assert L.bnn_mi355x_ecc_encode(0xABC1234) == 0x19  # (the low 16 bits are the element)
    assert L.bnn_mi355x_ecc_decode(1, 0x23, None) == 0
    # every network's library holds the same code
    for name in ("cnvW2A2", "lfcW1A1", "lfcW1A2"):
        assert gl.load(name).bnn_mi355x_ecc_encode(0x1234) == 0x19


def test_every_single_error_is_restored():
    L = gl.load("cnvW1A1")
    assert len(WORDS) >= 50
    for d in WORDS:
        c = L.bnn_mi355x_ecc_encode(d)
        for p in range(22):
            dm, cm = flips((p,))
            assert lib_decode(L, d ^ dm, c ^ cm) == (1, d), (hex(d), p)


def test_no_double_error_is_miscorrected():
    L = gl.load("cnvW1A1")
    pairs = list(itertools.combinations(range(22), 2))
    assert len(pairs) == 231
    for d in WORDS:
        c = L.bnn_mi355x_ecc_encode(d)
        for pq in pairs:
            dm, cm = flips(pq)
            assert lib_decode(L, d ^ dm, c ^ cm) == (2, d ^ dm), (hex(d), pq)


def test_triples_as_stated():
    """of the 1 540 triple errors 1 052 are accepted as a correction (and leave wrong data or a wrong check) and 488 are
    detected: a property of the definition, the same for the library and the restatement"""
    L = gl.load("cnvW1A1")
    got = {1: 0, 2: 0}
    for pqr in itertools.combinations(range(22), 3):
        dm, cm = flips(pqr)
        status, _ = lib_decode(L, dm, cm)
        assert status == er.decode(dm, cm)[0]
        got[status] += 1
    assert got == {1: 1052, 2: 488}


def test_library_against_the_restatement_and_linearity():
    """20 000 seeded random (data, data mask, check mask): the library's encode and decode are the restatement's, and the
    status and corrected bit of (d ^ dm, encode(d) ^ cm) are those of the error pattern (dm, cm) alone"""
    L = gl.load("lfcW1A1")
    rng = np.random.default_rng(1816)
    n = 20000
    data = rng.integers(0, 1 << 16, n).tolist()
    # (0 ... 4 error bits, or dense random masks)
    dmask, cmask = [], []
    for k in rng.integers(0, 6, n).tolist():
        dm, cm = flips(rng.choice(22, k, replace=False).tolist()) if k < 5 else (int(rng.integers(0, 1 << 16)), int(rng.integers(0, 64)))
        dmask.append(dm)
        cmask.append(cm)
    seen = {0: 0, 1: 0, 2: 0}
    for d, dm, cm in zip(data, dmask, cmask):
        c = L.bnn_mi355x_ecc_encode(d)
        assert c == er.encode(d)
        status, out = lib_decode(L, d ^ dm, c ^ cm)
        assert (status, out) == er.decode(d ^ dm, c ^ cm)
        s2, residual = lib_decode(L, dm, cm)
        assert s2 == status and out == d ^ residual, (hex(d), hex(dm), hex(cm))
        seen[status] += 1
    assert min(seen.values()) > 100
