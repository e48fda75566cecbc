"""bnn_mi355x_ecc_repair, host side (no GPU): what a repair scrub leaves stored of one code word (csrc/ecc.h), checked
exhaustively over the error patterns of weight 1, 2 and 3 on data words 0, 0xFFFF, 0x1234 and a few seeded ones, against
the code's definition (tests/ecc_ref.py: positions, not masks).  All 22 singles return to the code word; all 231 doubles
are left as stored with status 2; of the 1 540 triples 1 052 are rewritten to a valid code word with wrong data, which
decodes with status 0 from then on, and the other 488 are left; a repair is idempotent."""
import itertools

import numpy as np
import pytest

import ecc_ref as er
import gpu_lib as gl
import repair_ref as rr

WORDS = [0, 0xFFFF, 0x1234] + np.random.default_rng(19).integers(0, 1 << 16, 5).tolist()


def stored(d, positions):
    """code word of d with the given of its 22 positions (data bits 0 ... 15, check bits 16 ... 21) flipped"""
    m = sum(1 << p for p in positions)
    return d ^ (m & 0xFFFF), er.encode(d) ^ (m >> 16)


@pytest.fixture(scope="module")
def L():
    return gl.load("lfcW1A1")


def test_clean_words_are_left(L):
    for d in WORDS:
        assert rr.lib_repair(L, d, er.encode(d)) == (0, d, er.encode(d))
    # (arguments wider than the fields: only the low 16 and 6 bits are read or returned)
    assert rr.lib_repair(L, 0xABCD1234, 0xFFC0 | er.encode(0x1234)) == (0, 0x1234, er.encode(0x1234))
    assert L.bnn_mi355x_ecc_repair(1, 0, None, None) == 1


@pytest.mark.parametrize("d", WORDS)
def test_singles_return_to_the_code_word(L, d):
    for p in range(22):
        assert rr.lib_repair(L, *stored(d, (p,))) == (1, d, er.encode(d)), p


@pytest.mark.parametrize("d", WORDS)
def test_doubles_are_left_as_stored(L, d):
    pairs = list(itertools.combinations(range(22), 2))
    assert len(pairs) == 231
    for ps in pairs:
        sd, sc = stored(d, ps)
        assert rr.lib_repair(L, sd, sc) == (2, sd, sc), ps


@pytest.mark.parametrize("d", WORDS)
def test_triples_are_locked_in_or_left(L, d):
    triples = list(itertools.combinations(range(22), 3))
    assert len(triples) == 1540
    rewritten = left = 0
    for ps in triples:
        sd, sc = stored(d, ps)
        st, nd, nc = rr.lib_repair(L, sd, sc)
        assert (st, nd, nc) == rr.repair_word(sd, sc), ps
        if st == 1:  # accepted as a correction: a valid code word with wrong data, clean-looking from then on
            rewritten += 1
            assert nd != d and nc == er.encode(nd) and er.decode(nd, nc) == (0, nd)
            assert rr.lib_repair(L, nd, nc) == (0, nd, nc)
            assert bin((nd ^ d) | (nc ^ er.encode(d)) << 16).count("1") == 4  # (the nearest other code word)
        else:
            left += 1
            assert (st, nd, nc) == (2, sd, sc)
    assert (rewritten, left) == (1052, 488)


def test_repair_is_idempotent_and_agrees_with_decode(L):
    rng = np.random.default_rng(5)
    for sd, sc in zip(rng.integers(0, 1 << 16, 4000).tolist(), rng.integers(0, 64, 4000).tolist()):
        st, nd, nc = rr.lib_repair(L, sd, sc)
        assert (st, nd, nc) == rr.repair_word(sd, sc)
        assert er.decode(nd, nc)[1] == er.decode(sd, sc)[1]  # the delivered data is the same before and after
        again = rr.lib_repair(L, nd, nc)
        assert again[1:] == (nd, nc) and again[0] == (2 if st == 2 else 0)


def test_error_pattern_rule_is_the_statement_on_stored_words(L):
    """the code is linear: repairing the error pattern (dm, cm) and adding it to the code word is repairing the stored word"""
    rng = np.random.default_rng(6)
    for d in WORDS:
        for dm, cm in zip(rng.integers(0, 1 << 16, 300).tolist(), rng.integers(0, 64, 300).tolist()):
            if bin(dm).count("1") + bin(cm).count("1") > 3:
                dm, cm = dm & 0x0101, cm & 0x21
            st, m, mc = rr.lib_repair(L, dm, cm)
            assert rr.lib_repair(L, d ^ dm, er.encode(d) ^ cm) == (st, d ^ m, er.encode(d) ^ mc)
