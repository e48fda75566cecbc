"""GPU: CNV layers 4-7 of cnvW1A1, cnvW1A2 and cnvW2A2 on the matrix pipe (k_tail_mfma, DESIGN.md 5 "The matrix pipe").
Every bit of the four stages against the faithful scalar restatement on small batches (the policy forced down with
BNN_MI355X_TAIL_MFMA_MIN=1 and BNN_MI355X_CONV_MFMA_MIN=1; shipped and random parameter sets, cnvW2A2 also with -2
weights), which path a call takes (bits 4-7 of bnn_mi355x_matrix_stages -- the results cannot tell), the policy edge, the
forked 131 072-image pass against the integer-pipe kernels (BNN_MI355X_CONV=valu) byte for byte, the places where the blob
changes (a fault campaign's persistent row patches in layers 4-7, a blob imported from device memory), and cnvW1A1's
integer-pipe forms at the sizes the matrix forms have taken over.  The switches are read once per process: each
configuration runs in a child process, each child under its own timeout."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import dispatch_forms as df
import gpu_lib as gl

pytestmark = pytest.mark.gpu

TESTS = os.path.dirname(os.path.abspath(__file__))
NETS = ("cnvW1A1", "cnvW1A2", "cnvW2A2")
STAGES = ((4, 9, 256), (5, 1, 256), (6, 1, 512), (7, 1, 512))  # stage, pixels, channels
L123, L47 = 0b1110, 0xF0                                        # bnn_mi355x_matrix_stages: layers 1-3, layers 4-7
SWITCHES = ("BNN_MI355X_CONV", "BNN_MI355X_CONV_MFMA_MIN", "BNN_MI355X_TAIL_MFMA_MIN", "BNN_MI355X_L1", "BNN_MI355X_L0")


def planes(network):
    return 2 if network.endswith("A2") else 1


def prelude(network):
    return (
        "import sys, ctypes as C, numpy as np; sys.path[:0] = [%r, %r]\n"
        "import torch, gpu_lib as gl, oracle_lib as ol\n"
        "from test_gpu_layers import stage_output, unpack\n"
        "NET = %r\n"
        "PLANES = %d\n"
        "L = gl.load(NET)\n"
        "def load(pdir):\n"
        "    L.load_parameters(pdir.encode()); assert L.bnn_mi355x_last_error() == b''\n"
        "def net():\n"
        "    n = gl.Net.__new__(gl.Net); n.L, n.network, n.is_cnv, n.isz = L, NET, True, 3072\n"
        "    return n\n"
        "SHIPPED = gl.param_dir('cifar10', NET)\n" % (TESTS, os.path.join(gl.ROOT, "bnn-pynq_amd"), network, planes(network)))


def child(network, code, timeout=900, **env):
    e = dict(os.environ)
    for k in SWITCHES:
        e.pop(k, None)
    e.update({k: str(v) for k, v in env.items()})
    out = subprocess.run([sys.executable, "-c", prelude(network) + code + "\nprint('child-ok')\n"], env=e, capture_output=True, text=True,
                         timeout=timeout)
    assert "child-ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]
    return out.stdout


def policy_min(network):
    """the committed edge of `network` for layers 4-7"""
    with open(os.path.join(gl.ROOT, "bnn-pynq_amd", "csrc", "kernels.hip")) as f:
        src = f.read()
    m = re.search(r"constexpr long long kTailMfmaMinW1A1 = (\d+), kTailMfmaMinW1A2 = (\d+), kTailMfmaMinW2A2 = (\d+);", src)
    return int(m.group(1 + NETS.index(network)))


@pytest.mark.parametrize("network", NETS)
def test_stages_4_to_7_bit_exact_small_batches(network, tmp_path):
    """the matrix forms on 1, 2, 5, 33 and 203 images (ragged last groups and tiles of both item shapes: 9 items per
    image, 1 item per image), shipped and random parameters (unordered, never / always firing thresholds among them;
    cnvW2A2 also a set with -2 weights): every bit of stages 4-7 of images 0, n - 1 and every 7th against
    Oracle.layer_ref, and the whole network's raw scores on 3 001 images against scores_fast"""
    import random_params
    sets = [str(tmp_path / "r")]
    random_params.make(sets[0], network, 51)
    if network == "cnvW2A2":
        sets.append(str(tmp_path / "neg2"))
        random_params.make(sets[1], network, 52, neg2=0.03)
    child(network,
          "for pdir in [SHIPPED] + %r:\n"
          "    load(pdir); o = ol.Oracle(NET, pdir)\n"
          "    for n in (1, 2, 5, 33, 203):\n"
          "        assert L.bnn_mi355x_matrix_stages(n) & %d == %d\n"
          "        imgs = np.random.default_rng(80 + n).integers(0, 256, (n, 3072), dtype=np.uint8)\n"
          "        for stage, pixels, channels in %r:\n"
          "            raw = stage_output(L, imgs, stage)\n"
          "            for i in sorted({0, n - 1} | set(range(0, n, 7))):\n"
          "                assert (unpack(raw[i], pixels, channels, PLANES) == o.layer_ref(imgs[i], stage)).all(), (pdir, n, stage, i)\n"
          "    imgs = np.random.default_rng(9).integers(0, 256, (3001, 3072), dtype=np.uint8)\n"
          "    assert (net().raw(imgs) == o.scores_fast(imgs)).all(), pdir\n" % (sets, L47, L47, STAGES),
          BNN_MI355X_TAIL_MFMA_MIN=1, BNN_MI355X_CONV_MFMA_MIN=1)


@pytest.mark.parametrize("network", NETS)
def test_matrix_stages_reports_the_path(network):
    """bits 4-7 of bnn_mi355x_matrix_stages: set at the committed edge and at 8 192, 65 536 and 131 072, clear one image
    below the edge; clear everywhere under BNN_MI355X_CONV=valu and under BNN_MI355X_TAIL_MFMA_MIN=200000; set at 1 image
    under =1; -1 before load_parameters.  Bits 1-3 (layers 1-3) do not depend on the new switch."""
    m = policy_min(network)
    assert 1 < m <= 65536
    sizes = (1, m - 1, m, m + 1, 8192, 65536, 131072)
    want = [L47 if n >= m else 0 for n in sizes]
    assert want[1] == 0 and want[2] == L47 and want[4:] == [L47] * 3   # (the edge lies at or below 8 192)
    out = child(network,
                "assert L.bnn_mi355x_matrix_stages(%d) == -1\n"
                "load(SHIPPED)\n"
                "got = [L.bnn_mi355x_matrix_stages(n) for n in %r]\n"
                "assert [g & %d for g in got] == %r, got\n"
                "print('low', [g & 15 for g in got])\n" % (m, sizes, L47, want))
    low = re.search(r"low (\[.*?\])", out).group(1)
    child(network,
          "load(SHIPPED)\n"
          "for n in %r:\n"
          "    got = L.bnn_mi355x_matrix_stages(n)\n"
          "    assert got & 1 and got & %d == 0, (n, got)\n" % (sizes, L47 | L123), BNN_MI355X_CONV="valu")
    off = child(network,
                "load(SHIPPED)\n"
                "got = [L.bnn_mi355x_matrix_stages(n) for n in %r]\n"
                "assert all(g & %d == 0 for g in got), got\n"
                "print('low', [g & 15 for g in got])\n" % (sizes, L47), BNN_MI355X_TAIL_MFMA_MIN=200000)
    assert re.search(r"low (\[.*?\])", off).group(1) == low            # layers 0-3: untouched by the switch
    down = child(network,
                 "load(SHIPPED)\n"
                 "got = [L.bnn_mi355x_matrix_stages(n) for n in %r]\n"
                 "assert all(g & %d == %d for g in got) and L.bnn_mi355x_matrix_stages(0) == 0, got\n"
                 "print('low', [g & 15 for g in got])\n" % (sizes, L47, L47), BNN_MI355X_TAIL_MFMA_MIN=1)
    assert re.search(r"low (\[.*?\])", down).group(1) == low


@pytest.mark.parametrize("network", NETS)
def test_policy_edge(network):
    """edge - 1 images (integer-pipe kernels) against edge images (matrix forms): the same outputs of stages 4-7"""
    m = policy_min(network)
    assert 1 < m <= 65536
    child(network,
          "load(SHIPPED)\n"
          "assert L.bnn_mi355x_matrix_stages(%d) & %d == 0 and L.bnn_mi355x_matrix_stages(%d) & %d == %d\n"
          "imgs = np.random.default_rng(5).integers(0, 256, (%d, 3072), dtype=np.uint8)\n"
          "for stage, pixels, channels in %r:\n"
          "    a = stage_output(L, imgs[:-1], stage); b = stage_output(L, imgs, stage)\n"
          "    assert (a == b[:-1]).all(), stage\n" % (m - 1, L47, m, L47, L47, m, STAGES))


def _dump_forked(path):
    return (
        "load(SHIPPED)\n"
        "imgs = np.random.default_rng(13).integers(0, 256, (131072, 3072), dtype=np.uint8)\n"
        "d = torch.from_numpy(imgs).cuda(); cls = torch.zeros(131072, dtype=torch.int32, device='cuda')\n"
        "sc = torch.zeros((131072, 64), dtype=torch.int16, device='cuda')\n"
        "assert L.bnn_mi355x_inference_device(d.data_ptr(), 131072, 10, cls.data_ptr(), sc.data_ptr(), None, None) == 0\n"
        "torch.cuda.synchronize()\n"
        "st = [stage_output(L, imgs[:16384], s) for s, _, _ in %r]\n"
        "np.savez(%r, cls=cls.cpu().numpy(), sc=sc.cpu().numpy(), s4=st[0], s5=st[1], s6=st[2], s7=st[3])\n" % (STAGES, str(path)))


@pytest.mark.parametrize("network", NETS)
def test_forked_pass_equals_integer_pipe_kernels(network, tmp_path):
    """131 072 images through the device entry point (the pass forks over two lanes of 65 536): classes and all 64 raw
    scores equal those of the integer-pipe kernels byte for byte, stage 4-7 outputs of a 16 384-image host call too, and
    2 048 of the images equal the restatement"""
    child(network, "assert L.bnn_mi355x_matrix_stages(-1) == -1\n" + _dump_forked(tmp_path / "mfma.npz")
          + "assert L.bnn_mi355x_matrix_stages(65536) & %d == %d and L.bnn_mi355x_matrix_stages(16384) & %d == %d\n" % (L47, L47, L47, L47))
    child(network, _dump_forked(tmp_path / "valu.npz") + "assert L.bnn_mi355x_matrix_stages(65536) & %d == 0\n" % (L47 | L123),
          BNN_MI355X_CONV="valu")
    a, b = np.load(tmp_path / "mfma.npz"), np.load(tmp_path / "valu.npz")
    for k in ("cls", "sc", "s4", "s5", "s6", "s7"):
        assert (a[k] == b[k]).all(), k
    import oracle_lib as ol
    imgs = np.random.default_rng(13).integers(0, 256, (131072, 3072), dtype=np.uint8)
    pick = np.random.default_rng(1).choice(131072, 2048, replace=False)
    o = ol.Oracle(network, gl.param_dir("cifar10", network))
    assert (a["sc"][pick] == o.scores_fast(imgs[pick])).all()


def _after_faults(path, tmp):
    return (
        "load(SHIPPED)\n"
        "imgs = np.random.default_rng(21).integers(0, 256, (300, 3072), dtype=np.uint8)\n"
        "f = %r\n"
        "np.concatenate([np.ones((300, 1), np.uint8), imgs], axis=1).tofile(f)\n"
        "assert L.bnn_mi355x_set_fault_seed(78) == 0\n"
        "cnt = C.c_int(0)\n"
        "p = L.inference_multiple_with_faults(f.encode(), 10, C.byref(cnt), None, 400, 1, -1, (C.c_int * 4)(4, 5, 6, 7), 4)\n"
        "assert p and cnt.value == 300, L.bnn_mi355x_last_error()\n"
        "camp = np.ctypeslib.as_array(p, shape=(300,)).copy(); L.free_results(p)\n"
        "big = np.random.default_rng(22).integers(0, 256, (8192, 3072), dtype=np.uint8)\n"
        "np.savez(%r, camp=camp, sc=net().raw(big), stages=np.int32(L.bnn_mi355x_matrix_stages(8192)))\n" % (str(tmp / "imgs.bin"), str(path)))


@pytest.mark.parametrize("network", NETS)
def test_plain_call_after_fault_campaign(network, tmp_path):
    """inference_multiple_with_faults (400 single-bit faults targeted at layers 4-7, word size 1: in cnvW2A2 a flip of a
    field's low bit makes a -2 out of a -1) patches rows of those layers and the patches persist: the next plain call
    (matrix forms, 8 192 images, forced down so that every chunk takes them) classifies with the patched weights -- the
    same scores as under BNN_MI355X_CONV=valu, and the same campaign classes"""
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    child(network, _after_faults(tmp_path / "mfma.npz", tmp_path / "a"), BNN_MI355X_TAIL_MFMA_MIN=1, BNN_MI355X_CONV_MFMA_MIN=1)
    child(network, _after_faults(tmp_path / "valu.npz", tmp_path / "b"), BNN_MI355X_CONV="valu")
    a, b = np.load(tmp_path / "mfma.npz"), np.load(tmp_path / "valu.npz")
    assert int(a["stages"]) & L47 == L47 and int(b["stages"]) & L47 == 0
    assert (a["camp"] == b["camp"]).all()
    assert (a["sc"] == b["sc"]).all()


@pytest.mark.parametrize("network", NETS)
def test_blob_imported_from_device(network, tmp_path):
    """a random parameter set's blob imported from device memory (the host never sees the parameter files) gives the
    matrix forms the same tables as load_parameters: equal scores on 8 192 images, equal to the restatement"""
    import random_params
    random_params.make(str(tmp_path), network, 53, **({"neg2": 0.02} if network == "cnvW2A2" else {}))
    child(network,
          "pdir = %r\n"
          "imgs = np.random.default_rng(23).integers(0, 256, (8192, 3072), dtype=np.uint8)\n"
          "load(pdir); want = net().raw(imgs)\n"
          "load(SHIPPED)\n"
          "size = L.bnn_mi355x_params_bytes(); blob = gl.pack_params(NET, pdir); assert blob.size == size\n"
          "d = torch.from_numpy(blob).cuda()\n"
          "assert L.bnn_mi355x_import_params_device(d.data_ptr(), size, torch.cuda.current_stream().cuda_stream) == 0\n"
          "assert L.bnn_mi355x_matrix_stages(8192) & %d == %d\n"
          "got = net().raw(imgs)\n"
          "assert (got == want).all()\n"
          "assert (got[:512] == ol.Oracle(NET, pdir).scores_fast(imgs[:512])).all()\n" % (str(tmp_path), L47, L47),
          BNN_MI355X_TAIL_MFMA_MIN=1, BNN_MI355X_CONV_MFMA_MIN=1)


def test_integer_pipe_forms_of_cnvW1A1_at_the_policy_edges(tmp_path):
    """cnvW1A1's integer-pipe forms (BNN_MI355X_CONV=valu; still the path of every fault-injection entry point) at the
    sizes of dispatch_forms.edges() and the size before each: every image of every call equals the same image of the
    largest call, and the images below 1 100, the 64 either side of every call end and every 64th of the rest equal
    scores_fast.  (tests/test_gpu_conv_matrix_a2.py does the same for the 2-bit nets.)"""
    network = "cnvW1A1"
    sizes = sorted({x for e in df.edges(lambda n: df.cnv_forms(n, network)) for x in (e - 1, e)})
    keep = np.zeros(sizes[-1], bool)
    keep[:1100] = True
    keep[::64] = True
    for s in sizes:
        keep[max(s - 64, 0):s + 64] = True
    pick = np.nonzero(keep)[0]
    child(network,
          "load(SHIPPED)\n"
          "sizes = %r\n"
          "imgs = np.random.default_rng(31).integers(0, 256, (sizes[-1], 3072), dtype=np.uint8)\n"
          "ref = net().raw(imgs)\n"
          "for n in sizes[:-1]:\n"
          "    assert L.bnn_mi355x_matrix_stages(n) & %d == 0\n"
          "    assert (net().raw(imgs[:n]) == ref[:n]).all(), n\n"
          "np.save(%r, ref)\n" % (sizes, L47 | L123, str(tmp_path / "ref.npy")), BNN_MI355X_CONV="valu")
    import oracle_lib as ol
    ref = np.load(tmp_path / "ref.npy")
    imgs = np.random.default_rng(31).integers(0, 256, (sizes[-1], 3072), dtype=np.uint8)
    o = ol.Oracle(network, gl.param_dir("cifar10", network))
    assert (ref[pick] == o.scores_fast(imgs[pick])).all()
