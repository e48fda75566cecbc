"""Which kernel instantiations the batch-size policy runs, checked under a kernel trace (profiles/r05_dispatch_forms_kernel_trace.txt).

  BNN_MI355X_LANES=1 rocprofv3 --kernel-trace --stats -d DIR/lanes1 -o run -- python tools/dispatch_forms_trace.py lanes1
  rocprofv3 --kernel-trace --stats -d DIR/forked -o run -- python tools/dispatch_forms_trace.py forked
  python tools/dispatch_forms_trace.py report DIR > profiles/r05_dispatch_forms_kernel_trace.txt

lanes1: cnvW2A2 with -2 rows (random parameters) and cnvW1A2 at 29 099, 32 769 and 130 817 images, one pass each;
forked: one 131 072-image cnvW2A2 (-2 rows) call on the default path (two lanes of 65 536).  The report reads the tracer's
SQLite output (rocpd, its default format) and lists every dispatch of the library in start order, one block per call, each headed by the forms tests/dispatch_forms.py names."""
import glob
import os
import sqlite3
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [os.path.join(ROOT, "tests"), os.path.join(ROOT, "bnn-pynq_amd")]

SIZES = (29099, 32769, 130817)
CALLS = {"lanes1": [(net, n) for net in ("cnvW2A2-neg2", "cnvW1A2") for n in SIZES], "forked": [("cnvW2A2-neg2", 131072)]}


def run(mode):
    import torch
    import gpu_lib as gl
    import random_params
    pdir = tempfile.mkdtemp()
    random_params.make(pdir, "cnvW2A2", 5, neg2=0.03)
    n_max = max(n for _, n in CALLS[mode])
    d = torch.randint(0, 256, (n_max, 3072), dtype=torch.uint8, device="cuda")
    cls = torch.zeros(n_max, dtype=torch.int32, device="cuda")
    for name, n in CALLS[mode]:
        L = gl.load(name.split("-")[0])
        L.load_parameters((pdir if name.endswith("neg2") else gl.param_dir("cifar10", name)).encode())
        assert L.bnn_mi355x_inference_device(d.data_ptr(), n, 10, cls.data_ptr(), None, None, None) == 0, L.bnn_mi355x_last_error()
        torch.cuda.synchronize()
        print(name, n, "ok")


def report(top):
    import dispatch_forms as df
    for mode in ("lanes1", "forked"):
        paths = glob.glob(os.path.join(top, mode, "**", "*results.db"), recursive=True)
        assert len(paths) == 1, (mode, paths)
        db = sqlite3.connect(paths[0])
        rows = [r for r in db.execute("select name, grid_x, grid_y, workgroup_x, stream_id from kernels order by start") if "bnn::" in r[0]]
        print("== %s (%s) ==" % (mode, "BNN_MI355X_LANES=1" if mode == "lanes1" else "default: forked over two lanes"))
        used = set()
        for name, n in CALLS[mode]:
            lanes = df.fork_lanes(n) if mode == "forked" else (n,)
            print("-- %s, %d images" % (name, n))
            for m in lanes:
                # a lane's nine stages end in its layer-8 launch, whose grid gives its size (the library's load-time warm-up
                # calls and the other lane also appear in the trace): the eight launches before it on the same stream
                blocks = -(-m // 4) if m <= df.C["kFcLastWaveMax"] else -(-m // 2048) * 8
                j = next(j for j in range(len(rows)) if j not in used and "k_fclast" in rows[j][0] and rows[j][1] // rows[j][3] == blocks)
                lane = [k for k in range(j, -1, -1) if rows[k][4] == rows[j][4] and k not in used][:9][::-1]
                used |= set(lane)
                print("   lane of %d images, forms %s:" % (m, " ".join(df.cnv_forms(m, name.split("-")[0], name.endswith("neg2")))))
                for k in lane:
                    nm, gx, gy, wx, _ = rows[k]
                    print("   %6d x %-3d blocks of %4d  %s" % (gx // wx, gy, wx, nm))
        print("(and %d launches of the library's load-time warm-up calls)" % (len(rows) - len(used)))
        print()


if __name__ == "__main__":
    if sys.argv[1] == "report":
        report(sys.argv[2])
    else:
        run(sys.argv[1])
