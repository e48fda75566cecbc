"""CPU: the ABI of the column-interleaved coded weight memories (include/bnn_mi355x.h): the new symbols are in the header
and in abi.EXT with their argument types declared, a base and a variant library export them, and every refusal is reached
without a device -- before any device work -- and names its reason; the earlier families keep theirs word for word."""
import ctypes as C
import re

import pytest

import gpu_lib as gl
import hardened_ref as hr
from bnn import abi

ARGS = {"bnn_mi355x_iwecc_layout": 4, "bnn_mi355x_iwecc_site": 6, "bnn_mi355x_pack_params_iwecc": 9,
        "bnn_mi355x_iwecc_exposure_campaigns": 17, "bnn_mi355x_iwecc_exposure_params": 14, "bnn_mi355x_last_iwecc_exposure_counts": 2,
        "bnn_mi355x_last_iwecc_exposure_seeds": 2}
up = C.c_uint * 9
RW, RT = up(*[hr.q32(2.0 ** -8)] * 9), up(*([hr.q32(2.0 ** -8)] * 8 + [0]))
BAD_WI = b"weight_interleave must be 0 (none) or 1 (column-interleaved code words)"
NEEDS = b"weight_interleave 1 needs weight_code 1"
BAD_WC = b"weight_code must be 0 (none) or 1 (SEC-DED (72,64) over the weights of layers >= 1)"


def test_declared_in_the_header_and_in_abi():
    with open(gl.ROOT + "/include/bnn_mi355x.h") as f:
        src = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name, n in ARGS.items():
        m = re.search(r"\b%s\s*\(([^;{]*)\)\s*;" % name, src)
        assert m and len(m.group(1).split(",")) == n, name
        assert name in abi.EXT and abi.EXT.count(name) == 1
    assert "iwecc_exposure_mask" not in src  # (the events are weight_code 1's: there is no mask entry point of this family)


@pytest.mark.parametrize("network", ["cnvW1A1", "lfcW1A2", "cnvW1A1-TMR", "cnvW1A2-interleaved"])
def test_exported_with_argument_types(network, variant_libs):
    L = gl.load(network)
    for name, n in ARGS.items():
        assert hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == n, name
    assert not hasattr(L, "bnn_mi355x_iwecc_exposure_mask")
    assert L.bnn_mi355x_iwecc_exposure_campaigns.restype == C.POINTER(C.c_int)
    assert L.bnn_mi355x_iwecc_exposure_params.restype == C.c_size_t and L.bnn_mi355x_pack_params_iwecc.restype == C.c_size_t
    assert L.bnn_mi355x_last_iwecc_exposure_counts(None, 0) == 0 and L.bnn_mi355x_last_iwecc_exposure_seeds(None, 0) == 0
    out = (C.c_int * 4)()
    last = 8 if network.startswith("cnv") else 3
    assert L.bnn_mi355x_iwecc_layout(1, 1, last, out) == 0 and out[0] == 1 and out[2] == 8 and out[3] in (2, 8, 16)
    assert L.bnn_mi355x_iwecc_layout(1, 1, last, None) == 0  # (out may be NULL)


def test_refusals_need_no_device(tmp_path):
    """nothing is loaded and no device is looked for: each call returns NULL / 0 / -1 with its own reason"""
    L = gl.load("cnvW1A1")
    pdir = gl.param_dir("cifar10", "cnvW1A1").encode()
    path = tmp_path / "images.bin"
    with open(path, "wb") as f:
        f.truncate(48 * 3073)  # (a sparse file: nothing is read)
    path = str(path).encode()

    def campaign(scheme=1, code=0, wc=1, wi=1, burst=1, runs=1, seed=1, rw=RW, rt=RT, n=9, ei=12, every=0, repair=1, path=path):
        return L.bnn_mi355x_iwecc_exposure_campaigns(path, 10, scheme, code, wc, wi, burst, runs, seed, rw, rt, n, ei, every, repair, None, None)

    def params(scheme=1, code=0, wc=1, wi=1, burst=1, rw=RW, rt=RT, n=9, epoch=1, every=0, repair=1):
        return L.bnn_mi355x_iwecc_exposure_params(scheme, code, wc, wi, burst, 1, rw, rt, n, epoch, every, repair, None, 0)

    for kw, reason in ((dict(wi=2), BAD_WI), (dict(wi=-1), BAD_WI), (dict(wc=0, wi=1), NEEDS),
                       (dict(wc=2), BAD_WC), (dict(wc=2, wi=0), BAD_WC), (dict(wc=-1, wi=1), b"weight_code must be 0 (none) or 1"),
                       (dict(repair=-1), b"repair_every must not be negative"),
                       (dict(every=-1), b"scrub_every must not be negative"),
                       (dict(ei=0), b"epoch_images must be at least 1"),
                       (dict(scheme=1, code=1), b"TMR plus a code is not modelled"),
                       (dict(code=2), b"code must be 0 (none) or 1 (SEC-DED)"),
                       (dict(scheme=4), b"scheme must be"),
                       (dict(burst=17), b"burst must be 1 ... 16"),
                       (dict(n=8), b"one rate per layer"),
                       (dict(rw=None), b"a rate array missing"),
                       (dict(runs=0), b"num_runs must be"),
                       (dict(path=None), b"path missing"),
                       (dict(path=b"/nonexistent/images.bin"), b"Could not open file")):
        assert not campaign(**kw), kw
        assert reason in L.bnn_mi355x_last_error(), (kw, L.bnn_mi355x_last_error())
        assert b"iwecc_exposure_campaigns" in L.bnn_mi355x_last_error() or b"Could not open" in L.bnn_mi355x_last_error()
        assert L.bnn_mi355x_last_iwecc_exposure_counts(None, 0) == 0 and L.bnn_mi355x_last_iwecc_exposure_seeds(None, 0) == 0
        kw = {k: v for k, v in kw.items() if k in ("scheme", "code", "wc", "wi", "burst", "rw", "rt", "n", "every", "repair")}
        if kw:
            assert params(**kw) == 0, kw
            assert reason in L.bnn_mi355x_last_error() and b"iwecc_exposure_params" in L.bnn_mi355x_last_error(), (kw, L.bnn_mi355x_last_error())
    assert params(epoch=-1) == 0 and b"epoch must be 0 ..." in L.bnn_mi355x_last_error()
    # the host-only entry points
    out4, out2 = (C.c_int * 4)(), (C.c_long * 2)()
    for wc, wi, reason in ((1, 2, BAD_WI), (0, 1, NEEDS), (2, 1, BAD_WC), (2, 0, BAD_WC)):
        assert L.bnn_mi355x_iwecc_layout(wc, wi, 1, out4) == -1 and b"iwecc_layout: " + reason in L.bnn_mi355x_last_error()
        assert L.bnn_mi355x_iwecc_site(wc, wi, 1, 0, 0, out2) == -1 and b"iwecc_site: " + reason in L.bnn_mi355x_last_error()
        assert L.bnn_mi355x_pack_params_iwecc(pdir, 0, 0, wc, wi, None, 0, None, 0) == 0
        assert b"pack_params_iwecc: " + reason in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_iwecc_layout(1, 1, 9, out4) == -1 and b"iwecc_layout: layer must be 0 ... 8" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_iwecc_site(1, 1, -1, 0, 0, out2) == -1 and b"iwecc_site: layer must be 0 ... 8" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_iwecc_site(1, 1, 1, 2, 0, out2) == -1 and b"iwecc_site: module must be 0" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_iwecc_site(1, 1, 0, 0, 0, out2) == -1 and b"iwecc_site: the weight memory of layer 0 is not coded" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_iwecc_site(0, 0, 1, 0, 0, out2) == -1 and b"is not coded" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_iwecc_site(1, 1, 1, 0, -1, out2) == -1 and b"iwecc_site: index must be 0 ... " in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_iwecc_site(1, 1, 1, 1, 1 << 40, out2) == -1 and b"iwecc_site: index must be 0 ... " in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_pack_params_iwecc(pdir, 1, 1, 1, 1, None, 0, None, 0) == 0
    assert b"pack_params_iwecc: code 1 with scheme 1 (TMR)" in L.bnn_mi355x_last_error()
    # the earlier families keep their refusals word for word
    assert not L.bnn_mi355x_wecc_exposure_campaigns(path, 10, 1, 0, 2, 1, 1, 1, RW, RT, 9, 12, 0, 1, None, None)
    assert L.bnn_mi355x_last_error() == b"wecc_exposure_campaigns: " + BAD_WC
    assert L.bnn_mi355x_wecc_exposure_params(1, 0, 2, 1, 1, RW, RT, 9, 1, 0, 1, None, 0) == 0
    assert L.bnn_mi355x_last_error() == b"wecc_exposure_params: " + BAD_WC
    assert L.bnn_mi355x_pack_params_wecc(pdir, 1, 1, 1, None, 0, None, 0) == 0
    assert b"pack_params_wecc: code 1 with scheme 1 (TMR)" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_wecc_layout(2, 1, None) == -1 and L.bnn_mi355x_last_error() == b"wecc_layout: " + BAD_WC
    assert L.bnn_mi355x_pack_params_repair(pdir, 1, 1, None, 0, None, 0) == 0
    assert b"pack_params_repair: code 1 with scheme 1 (TMR)" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_ecc_exposure_mask(0, 0, 17, 1, 0, 1, 0, 0, 1, 0, None, 0) == -1
    assert b"ecc_exposure_mask: bad burst" in L.bnn_mi355x_last_error()
    assert L.bnn_mi355x_wecc_exposure_mask(0, 0, 1, 17, 1, 0, 1, 0, 0, 1, 0, None, 0) == -1
    assert b"wecc_exposure_mask: bad burst" in L.bnn_mi355x_last_error()


def test_past_the_refusals_it_is_the_device_that_is_missing(tmp_path):
    """with every argument in order the next step is the device: on a machine without one the call fails there, not before"""
    try:
        import torch
        if torch.cuda.is_available():
            return  # (a device is there: tests/test_gpu_iwecc_exposure.py runs the call)
    except ImportError:
        pass
    L = gl.load("cnvW2A2")
    path = tmp_path / "images.bin"
    with open(path, "wb") as f:
        f.truncate(48 * 3073)
    assert not L.bnn_mi355x_iwecc_exposure_campaigns(str(path).encode(), 10, 1, 0, 1, 1, 1, 1, 1, RW, RT, 9, 12, 0, 1, None, None)
    err = L.bnn_mi355x_last_error()
    assert err and b"weight_" not in err and b"counters" not in err and b"scheme" not in err
