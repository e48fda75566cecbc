"""The SEC-DED (72,64) code of the weight memories, host side (no GPU): bnn_mi355x_wecc_encode / _wecc_decode /
_wecc_repair (csrc/wecc.h) against the plain-Python statement of tests/wecc_ref.py, exhaustively over the error patterns
of weight <= 3 on a few random data words.  All checks are exact."""
import itertools
import random

import numpy as np

import gpu_lib as gl
import wecc_ref as wr

M64 = (1 << 64) - 1
WORDS = [0, M64, 0x0123456789ABCDEF] + [random.Random(20261121 + i).getrandbits(64) for i in range(3)]


def lib():
    return gl.load("lfcW1A1")


def split(mask72):
    """error positions 0 ... 63 the data bits, 64 ... 71 the check bits"""
    return mask72 & M64, mask72 >> 64


def test_encode_matches_the_definition_and_every_word_has_even_weight():
    L = lib()
    rng = random.Random(1)
    for d in WORDS + [1 << k for k in range(64)] + [rng.getrandbits(64) for _ in range(200)]:
        c = wr.encode(d)
        assert L.bnn_mi355x_wecc_encode(d) == c
        assert (bin(d).count("1") + bin(c).count("1")) % 2 == 0
        assert wr.lib_decode(L, d, c) == (0, d) == wr.decode(d, c)
    arr = np.array(WORDS, np.uint64)
    assert wr.encode_all(arr).tolist() == [wr.encode(d) for d in WORDS]


def test_all_72_single_errors_are_restored():
    L = lib()
    for d in WORDS:
        c = wr.encode(d)
        for k in range(72):
            dm, cm = split(1 << k)
            assert wr.lib_decode(L, d ^ dm, c ^ cm) == (1, d), (hex(d), k)
            assert wr.lib_repair(L, d ^ dm, c ^ cm) == (1, d, c)


def test_none_of_the_2556_double_errors_is_miscorrected():
    L = lib()
    pairs = list(itertools.combinations(range(72), 2))
    assert len(pairs) == 2556
    for d in WORDS[:3]:
        c = wr.encode(d)
        for a, b in pairs:
            dm, cm = split(1 << a | 1 << b)
            assert wr.lib_decode(L, d ^ dm, c ^ cm) == (2, d ^ dm), (hex(d), a, b)
            assert wr.lib_repair(L, d ^ dm, c ^ cm) == (2, d ^ dm, c ^ cm)


def test_triples_are_accepted_or_detected_and_linearity():
    """every triple is either accepted as a correction (status 1, a valid code word after the repair) or detected (status
    2, as stored); the two counts are the plain-Python statement's; status and remaining error depend on the error
    pattern alone: decode(d ^ dm, encode(d) ^ cm) = (status of decode(dm, cm), d ^ data of decode(dm, cm))"""
    L = lib()
    triples = list(itertools.combinations(range(72), 3))
    assert len(triples) == 59640
    patterns = np.array([sum(1 << k for k in t) for t in triples], object)
    dm = np.array([int(p) & M64 for p in patterns], np.uint64)
    cm = np.array([int(p) >> 64 for p in patterns], np.int64)
    status, rem = wr.decode_all(dm, cm)
    want = (int((status == 1).sum()), int((status == 2).sum()))
    assert sum(want) == len(triples) and want[0] > 0 and want[1] > 0
    accepted = detected = 0
    d = WORDS[3]
    c = wr.encode(d)
    for i, t in enumerate(triples):
        st, out = wr.lib_decode(L, int(dm[i]), int(cm[i]))
        assert (st, out) == (int(status[i]), int(rem[i])), t
        if i % 7 == 0:  # (the plain statement word by word, and the identity on a stored word)
            assert wr.decode(int(dm[i]), int(cm[i])) == (st, out)
            assert wr.lib_decode(L, d ^ int(dm[i]), c ^ int(cm[i])) == (st, d ^ out)
        if st == 1:
            accepted += 1
            assert out != 0  # (a triple is never restored: the data is wrong)
            rs, rd, rc = wr.lib_repair(L, d ^ int(dm[i]), c ^ int(cm[i]))
            assert rs == 1 and rd == d ^ out and rc == wr.encode(rd) and wr.lib_decode(L, rd, rc) == (0, rd)
        else:
            assert st == 2 and out == int(dm[i])
            detected += 1
    assert (accepted, detected) == want
    print("triples accepted %d detected %d" % want)


def test_repair_rule_on_error_patterns():
    """(dm, cm) -> (m, encode(m)) where decode(dm, cm) = (1, m), else unchanged: random patterns of weight 0 ... 5"""
    L = lib()
    rng = random.Random(5)
    for _ in range(3000):
        p = sum(1 << k for k in rng.sample(range(72), rng.randrange(6)))
        dm, cm = split(p)
        st, m = wr.decode(dm, cm)
        want = (1, m, wr.encode(m)) if st == 1 else (st, dm, cm)
        assert wr.lib_repair(L, dm, cm) == want == wr.repair_word(dm, cm)
        if st == 1:
            assert wr.lib_decode(L, want[1], want[2]) == (0, m)
