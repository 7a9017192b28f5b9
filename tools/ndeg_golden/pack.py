#!/usr/bin/env python3
"""tools/ndeg_golden/pack.py — TEST INFRASTRUCTURE, run by hand where the reference sources are present; nothing else runs it.

Builds ndeg_driver.cpp against the objects that `make -C oracle ref` leaves in oracle/_ref/ (with the flags of that recipe),
runs it for 4x4x4x4 and 6x4x2x8 and packs the result into tests/golden/ndeg_<X>x<Y>x<Z>x<T>.pK.npz: the parameters
(kappa, mu, epsilon), spinor2 and the 26 reference outputs, spread over parts that each stay below the size limit of a
committed file.  The gauge field is not packed: the driver's links are compared here with the committed ref_<dims>.npz.

(The name does not start with ref_: tests/qa_cases.py globs ref_*x*.npz for the files of the degenerate cases.)

  python3 tools/ndeg_golden/pack.py <directory of the reference sources>
"""
import glob
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
ORACLE = os.path.join(ROOT, "oracle")
GOLD = os.path.join(ROOT, "tests", "golden")
LATTICES = [(4, 4, 4, 4), (6, 4, 2, 8)]
PART_BYTES = 900 * 1024
REF_OBJS = ["t_wilson_dslash_reference", "t_clover_reference", "t_blas_reference", "t_test_util", "t_misc", "l_comm_single", "l_comm_common",
            "l_util_quda", "l_malloc"]


def build(ref, exe):
    subprocess.check_call(["make", "-C", ORACLE, "ref", "REF=" + ref])
    import triton
    cuda_inc = os.path.join(os.path.dirname(triton.__file__), "backends", "nvidia", "include")
    objs = [os.path.join(ORACLE, "_ref", o + ".o") for o in REF_OBJS]
    subprocess.check_call(["g++", "-std=c++11", "-O2", "-w", "-I" + ref + "/include", "-I" + ref + "/tests", "-I" + ref + "/lib", "-I" + cuda_inc,
                           os.path.join(HERE, "ndeg_driver.cpp")] + objs + ["-o", exe, "-fopenmp", "-lm", "-Wl,--unresolved-symbols=ignore-all"])


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    with tempfile.TemporaryDirectory() as work:
        exe = os.path.join(work, "ndeg_driver")
        build(ref, exe)
        for X in LATTICES:
            d = os.path.join(work, "%dx%dx%dx%d" % X)
            os.makedirs(d)
            subprocess.check_call([exe, d] + [str(x) for x in X])
            arrays = {}
            with open(os.path.join(d, "manifest.txt")) as f:
                header = f.readline().split()
                for line in f:
                    name, n = line.split()
                    a = np.fromfile(os.path.join(d, name + ".f64"), dtype="<f8")
                    assert a.size == int(n)
                    arrays[name] = a
            committed = np.load(os.path.join(GOLD, "ref_%dx%dx%dx%d.npz" % X))
            for mu in range(4):
                assert np.array_equal(arrays.pop("check_gauge%d" % mu), committed["gauge%d" % mu]), "the driver's links differ from the committed ones"
            assert np.array_equal(arrays["spinor2"][:committed["spinor"].size], committed["spinor"])
            outputs = sorted(k for k in arrays if k.startswith("ndeg_"))
            assert len(outputs) == 26, len(outputs)
            meta = dict(meta_X=np.array([int(v) for v in header[2:6]], dtype=np.int32), kappa=np.array(float(header[7])), mu=np.array(float(header[9])),
                        epsilon=np.array(float(header[11])))
            for old in glob.glob(os.path.join(GOLD, "ndeg_%dx%dx%dx%d.p*.npz" % X)):
                os.remove(old)
            parts, size = [dict(meta)], 0
            for k in ["spinor2"] + outputs:
                if size + arrays[k].nbytes > PART_BYTES:
                    parts.append({})
                    size = 0
                parts[-1][k] = arrays[k]
                size += arrays[k].nbytes
            for i, part in enumerate(parts):
                out = os.path.join(GOLD, "ndeg_%dx%dx%dx%d.p%d.npz" % (X + (i,)))
                np.savez_compressed(out, **part)
                assert os.path.getsize(out) < (1 << 20), out
                print("wrote", out, "%d arrays, %.2f MB" % (len(part), os.path.getsize(out) / 1e6))


if __name__ == "__main__":
    main()
