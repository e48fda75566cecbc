"""CPU: the ABI of the coded weight memories (include/bnn_mi355x.h): the new symbols are in the header and in abi.EXT with
their argument types declared, a base and a variant library export them, and every refusal is reached without a device --
before any device work -- and names its reason."""
import ctypes as C
import re

import pytest

import gpu_lib as gl
import hardened_ref as hr
from bnn import abi

ARGS = {"bnn_mi355x_wecc_encode": 1, "bnn_mi355x_wecc_decode": 3, "bnn_mi355x_wecc_repair": 4, "bnn_mi355x_wecc_layout": 3,
        "bnn_mi355x_wecc_exposure_mask": 13, "bnn_mi355x_pack_params_wecc": 8, "bnn_mi355x_wecc_exposure_campaigns": 16,
        "bnn_mi355x_wecc_exposure_params": 13, "bnn_mi355x_last_wecc_exposure_counts": 2, "bnn_mi355x_last_wecc_exposure_seeds": 2}
up = C.c_uint * 9
RW, RT = up(*[hr.q32(2.0 ** -8)] * 9), up(*([hr.q32(2.0 ** -8)] * 8 + [0]))


def test_declared_in_the_header_and_in_abi():
    with open(gl.ROOT + "/include/bnn_mi355x.h") as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name, n in ARGS.items():
        m = re.search(r"\b%s\s*\(([^;{]*)\)\s*;" % name, src)
        assert m and len(m.group(1).split(",")) == n, name
        assert name in abi.EXT and abi.EXT.count(name) == 1


@pytest.mark.parametrize("network", ["cnvW1A1", "lfcW1A2", "cnvW1A1-TMR", "cnvW1A2-interleaved"])
def test_exported_with_argument_types(network, variant_libs):
    L = gl.load(network)
    for name, n in ARGS.items():
        assert hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == n, name
    assert L.bnn_mi355x_wecc_exposure_campaigns.restype == C.POINTER(C.c_int)
    assert L.bnn_mi355x_wecc_exposure_params.restype == C.c_size_t and L.bnn_mi355x_pack_params_wecc.restype == C.c_size_t
    assert L.bnn_mi355x_wecc_exposure_mask.restype == C.c_long
    assert L.bnn_mi355x_last_wecc_exposure_counts(None, 0) == 0 and L.bnn_mi355x_last_wecc_exposure_seeds(None, 0) == 0
    d, c = C.c_ulonglong(0), C.c_uint(0)
    word = 0x0123456789ABCDEF
    assert L.bnn_mi355x_wecc_repair(word ^ (1 << 63), L.bnn_mi355x_wecc_encode(word), C.byref(d), C.byref(c)) == 1
    assert (d.value, c.value) == (word, L.bnn_mi355x_wecc_encode(word))
    assert L.bnn_mi355x_wecc_decode(word, L.bnn_mi355x_wecc_encode(word) ^ 0x80, None) == 1  # (out_data may be NULL)


def test_refusals_need_no_device(tmp_path):
    """nothing is loaded and no device is looked for: each call returns NULL / 0 with its own reason"""
    L = gl.load("cnvW1A1")
    path = tmp_path / "images.bin"
    with open(path, "wb") as f:
        f.truncate(48 * 3073)  # (a sparse file: nothing is read)
    path = str(path).encode()

    def campaign(scheme=1, code=0, wc=1, burst=1, runs=1, seed=1, rw=RW, rt=RT, n=9, ei=12, every=0, repair=1, path=path):
        return L.bnn_mi355x_wecc_exposure_campaigns(path, 10, scheme, code, wc, burst, runs, seed, rw, rt, n, ei, every, repair, None, None)

    def params(scheme=1, code=0, wc=1, burst=1, rw=RW, rt=RT, n=9, epoch=1, every=0, repair=1):
        return L.bnn_mi355x_wecc_exposure_params(scheme, code, wc, burst, 1, rw, rt, n, epoch, every, repair, None, 0)

    thresholds_in_the_last_layer = up(*[1] * 9)
    for kw, reason in ((dict(wc=2), b"weight_code must be 0 (none) or 1 (SEC-DED (72,64) over the weights of layers >= 1)"),
                       (dict(wc=-1), b"weight_code must be 0 (none) or 1"),
                       (dict(repair=-1), b"repair_every must not be negative"),
                       (dict(every=-1), b"scrub_every must not be negative"),
                       (dict(ei=0), b"epoch_images must be at least 1"),
                       (dict(scheme=1, code=1), b"TMR plus a code is not modelled"),
                       (dict(scheme=3, code=1), b"resilient patterns are defined for 32 and 48 positions only"),
                       (dict(code=2), b"code must be 0 (none) or 1 (SEC-DED)"),
                       (dict(scheme=4), b"scheme must be"),
                       (dict(burst=0), b"burst must be 1 ... 16"),
                       (dict(burst=17), b"burst must be 1 ... 16"),
                       (dict(n=8), b"one rate per layer"),
                       (dict(rw=None), b"a rate array missing"),
                       (dict(rt=thresholds_in_the_last_layer), b"layer 8 has no threshold memory"),
                       (dict(runs=0), b"num_runs must be"),
                       (dict(seed=(1 << 64) - 1, runs=2), b"seed + run wraps to 0"),
                       (dict(path=None), b"path missing"),
                       (dict(path=b"/nonexistent/images.bin"), b"Could not open file")):
        assert not campaign(**kw), kw
        assert reason in L.bnn_mi355x_last_error(), (kw, L.bnn_mi355x_last_error())
        assert b"wecc_exposure_campaigns" in L.bnn_mi355x_last_error() or b"Could not open" in L.bnn_mi355x_last_error()
        assert L.bnn_mi355x_last_wecc_exposure_counts(None, 0) == 0 and L.bnn_mi355x_last_wecc_exposure_seeds(None, 0) == 0
        kw = {k: v for k, v in kw.items() if k in ("scheme", "code", "wc", "burst", "rw", "rt", "n", "every", "repair")}
        if kw:
            assert params(**kw) == 0, kw
            assert reason in L.bnn_mi355x_last_error() and b"wecc_exposure_params" in L.bnn_mi355x_last_error(), (kw, L.bnn_mi355x_last_error())
    assert params(epoch=-1) == 0 and b"epoch must be 0 ..." in L.bnn_mi355x_last_error()
    assert params(epoch=1 << 16) == 0 and b"epoch must be 0 ..." in L.bnn_mi355x_last_error()
    # num_runs * E * layers * 12 >= 2^31, from the file's size alone: 2^15 epochs x 1024 runs x 9 layers x 12
    big = tmp_path / "sparse.bin"
    with open(big, "wb") as f:
        f.truncate((1 << 15) * 3073)
    assert not campaign(path=str(big).encode(), runs=1024, ei=1)
    assert b"num_runs * epochs * layers * 12 counters must stay below 2^31" in L.bnn_mi355x_last_error()
    assert not campaign(path=str(big).encode(), runs=1024, ei=1, wc=0, repair=0)  # (the route's own bound, with weight_code 0 as well)
    assert b"layers * 12 counters" in L.bnn_mi355x_last_error()
    # a (scheme, code) the network does not support
    W = gl.load("cnvW2A2")
    assert not W.bnn_mi355x_wecc_exposure_campaigns(path, 10, 2, 0, 1, 1, 1, 1, RW, RT, 9, 12, 0, 1, None, None)
    assert b"cnvW2A2 with scheme 2" in W.bnn_mi355x_last_error()
    F = gl.load("lfcW1A1")
    assert F.bnn_mi355x_wecc_exposure_params(1, 0, 1, 1, 1, RW, RT, 4, 1, 0, 1, None, 0) == 0
    assert b"LFC networks" in F.bnn_mi355x_last_error()
    # the earlier entry points keep their refusals word for word
    assert L.bnn_mi355x_pack_params_repair(gl.param_dir("cifar10", "cnvW1A1").encode(), 1, 1, None, 0, None, 0) == 0
    assert b"pack_params_repair: code 1 with scheme 1 (TMR)" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_ecc_exposure_mask(0, 0, 17, 1, 0, 1, 0, 0, 1, 0, None, 0) == -1
    assert b"ecc_exposure_mask: bad burst" in L.bnn_mi355x_last_error()


def test_past_the_refusals_it_is_the_device_that_is_missing(tmp_path):
    """with every argument in order the next step is the device: on a machine without one the call fails there, not before"""
    try:
        import torch
        if torch.cuda.is_available():
            return  # (a device is there: tests/test_gpu_wecc_exposure.py runs the call)
    except ImportError:
        pass
    L = gl.load("cnvW2A2")
    path = tmp_path / "images.bin"
    with open(path, "wb") as f:
        f.truncate(48 * 3073)
    assert not L.bnn_mi355x_wecc_exposure_campaigns(str(path).encode(), 10, 1, 0, 1, 1, 1, 1, RW, RT, 9, 12, 0, 1, None, None)
    err = L.bnn_mi355x_last_error()
    assert err and b"weight_code" not in err and b"counters" not in err and b"scheme" not in err
