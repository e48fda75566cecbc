"""CPU: the propagation-profile switch of the single-fault sweeps (bnn_mi355x_sweep_profile /
bnn_mi355x_last_sweep_profile) as far as it goes without a device -- the setting and what it returns, the empty profile,
the refusals -- the two k_sweep_profile instantiations in the BUILT gfx950 code object (no scratch, no spills), and the
reduction of a profile to masking curves (bnn.faults.propagation_curves) on hand-made arrays."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import gpu_lib as gl
from test_act_window_build import kernel_body, metadata
from test_conv_matrix_build import code_object  # noqa: F401  (the fixture)

sys.path.insert(0, os.path.join(gl.ROOT, "bnn-pynq_amd"))
lp = C.POINTER(C.c_long)
NETWORK = "cnvW1A2"  # (a library no GPU test profiles with: the state below is the process's)


def test_the_switch_returns_the_previous_setting():
    L = gl.load(NETWORK)
    try:
        assert L.bnn_mi355x_sweep_profile(1) == 0
        assert L.bnn_mi355x_sweep_profile(1) == 1
        assert L.bnn_mi355x_sweep_profile(0) == 1
        assert L.bnn_mi355x_sweep_profile(0) == 0
        assert L.bnn_mi355x_sweep_profile(7) == 0 and L.bnn_mi355x_sweep_profile(0) == 1  # (any non-zero value is on)
    finally:
        L.bnn_mi355x_sweep_profile(0)


def test_no_profile_before_a_sweep_and_a_negative_first():
    L = gl.load(NETWORK)
    cols = C.c_int(-1)
    assert L.bnn_mi355x_last_sweep_profile(0, None, None, 0, C.byref(cols)) == 0
    assert cols.value == 8  # (layers - 1 of a CNV network, profile or none)
    a, f = np.full(8, -3, np.int64), np.full(8, -3, np.int64)
    assert L.bnn_mi355x_last_sweep_profile(0, a.ctypes.data_as(lp), f.ctypes.data_as(lp), 1, None) == 0
    assert (a == -3).all() and (f == -3).all()  # (no rows: nothing written)
    cols = C.c_int(-1)
    assert gl.load("lfcW1A1").bnn_mi355x_last_sweep_profile(5, None, None, 0, C.byref(cols)) >= 0 and cols.value == 3
    assert L.bnn_mi355x_last_sweep_profile(-1, None, None, 0, None) == -1
    assert b"last_sweep_profile" in L.bnn_mi355x_last_error()


def sweeps(L):
    """one call of each of the three sweeps on a file that is not there, profiled or not: all three fail"""
    ch = (C.c_int * 1)()
    fault, site, bit = (C.c_int * 8)(0, 0, 1, 0, 0, 0, 0, 1), (C.c_int * 5)(0, 0, 0, 0, 1), (C.c_int * 2)(0, 7)
    return [L.bnn_mi355x_fault_sweep(b"/nonexistent", 10, fault, 1, ch, None, 0, None, None),
            L.bnn_mi355x_act_fault_sweep(b"/nonexistent", 10, site, 1, ch, None, 0, None, None),
            L.bnn_mi355x_input_fault_sweep(b"/nonexistent", 10, bit, 1, ch, None, 0, None, None)]


def test_a_profiled_sweep_that_fails_leaves_no_profile():
    """without a device (or, with one, without the file) every sweep fails, and with profiling on none leaves a profile"""
    L = gl.load(NETWORK)
    before = L.bnn_mi355x_sweep_profile(1)
    try:
        assert sweeps(L) == [-1, -1, -1]
        assert L.bnn_mi355x_last_error() != b""
        assert L.bnn_mi355x_last_sweep_profile(0, None, None, 0, None) == 0
    finally:
        L.bnn_mi355x_sweep_profile(before)


def test_no_gpu_fails_loudly():
    """a real file, parameters named: without a HIP device the profiled sweep refuses to compute like the plain one"""
    try:
        import torch
        if torch.cuda.is_available():
            pytest.skip("GPU present")
    except ImportError:
        pass
    L = gl.load("lfcW1A1")
    L.load_parameters(gl.param_dir("mnist", "lfcW1A1").encode())
    path = os.path.join(gl.ROOT, "tests", "golden", "3.image-idx3-ubyte").encode()
    rec, ch = (C.c_int * 2)(0, 7), (C.c_int * 1)()
    before = L.bnn_mi355x_sweep_profile(1)
    try:
        assert L.bnn_mi355x_input_fault_sweep(path, 10, rec, 1, ch, None, 0, None, None) == -1
        assert L.bnn_mi355x_last_error() != b""
        assert L.bnn_mi355x_last_sweep_profile(0, None, None, 0, None) == 0
    finally:
        L.bnn_mi355x_sweep_profile(before)


def test_variants_refused_profiled_or_not(variant_libs):
    """the hardened overlays: "not modelled" by all three sweeps, whatever the switch says"""
    for name in ("cnvW1A1-TMR", "lfcW1A2-interleaved"):
        L = gl.load(name)
        for on in (0, 1):
            before = L.bnn_mi355x_sweep_profile(on)
            try:
                assert sweeps(L) == [-1, -1, -1]
                assert b"not modelled" in L.bnn_mi355x_last_error()
                assert L.bnn_mi355x_last_sweep_profile(0, None, None, 0, None) == 0
            finally:
                L.bnn_mi355x_sweep_profile(before)


@pytest.mark.parametrize("name", ["k_sweep_profile<true>", "k_sweep_profile<false>"])
def test_profile_kernels_in_the_code_object(code_object, name):  # noqa: F811
    dis, notes = code_object
    body = kernel_body(dis, name)
    assert not re.search(r"\bscratch_|\bbuffer_store", body), "scratch traffic"
    md = metadata(notes, name)
    assert md["private_segment_fixed_size"] == 0 and md["vgpr_spill_count"] == 0 and md["sgpr_spill_count"] == 0
    assert md["group_segment_fixed_size"] == 16 and md["max_flat_workgroup_size"] == 256  # (a count per wave)
    assert md["vgpr_count"] + md.get("agpr_count", 0) <= 64  # (memory-bound: eight waves a SIMD)
    # 16-byte loads of both rows, the counters by 64-bit vector atomics
    assert len(re.findall(r"\bglobal_load_dwordx4\b", body)) >= 2
    assert len(re.findall(r"\bglobal_atomic_add_x2\b", body)) == 2


def test_python_binding_declares_both():
    L = gl.load(NETWORK)
    assert "bnn_mi355x_sweep_profile" in gl.EXT and "bnn_mi355x_last_sweep_profile" in gl.EXT
    assert L.bnn_mi355x_last_sweep_profile.restype is C.c_long
    from bnn import bnn as pkg
    assert callable(pkg.PynqBNN.sweep_profile) and callable(pkg.PynqBNN.last_sweep_profile)


def test_propagation_curves_on_hand_made_arrays():
    from bnn.faults.faults import propagation_curves
    # four faults on 10 images, three layers; fault 2 is never alive, fault 3 dies after the first layer
    alive = np.array([[10, 5, 1], [4, 4, 0], [0, 0, 0], [6, 0, 0]])
    flipped = np.array([[40, 5, 3], [4, 12, 0], [0, 0, 0], [9, 0, 0]])
    share, sizes = propagation_curves(alive, flipped, 10)
    assert share == [20 / 40.0, 9 / 40.0, 1 / 40.0]
    assert sizes == [(4.0 + 1.0 + 1.5) / 3, (1.0 + 3.0) / 2, 3.0]
    # from the second column on (faults of layer 1: the first column is not evaluated)
    share, size = propagation_curves(alive, flipped, 10, first=1)
    assert share == [9 / 40.0, 1 / 40.0] and size == [2.0, 3.0]
    # nothing alive anywhere: shares and sizes 0, no division by zero
    share, size = propagation_curves(np.zeros((3, 2), np.int64), np.zeros((3, 2), np.int64), 37)
    assert share == [0.0, 0.0] and size == [0.0, 0.0]
    # no faults, no images, every column cut off
    assert propagation_curves(np.zeros((0, 3), np.int64), np.zeros((0, 3), np.int64), 37) == ([0.0] * 3, [0.0] * 3)
    assert propagation_curves(alive, flipped, 0) == ([0.0] * 3, sizes)  # (the sizes need no image count)
    assert propagation_curves(alive, flipped, 10, first=3) == ([], [])
    # 64-bit counts stay exact
    big = np.array([[131072]]), np.array([[131072 * 57600]])
    assert propagation_curves(big[0], big[1], 131072) == ([1.0], [57600.0])
