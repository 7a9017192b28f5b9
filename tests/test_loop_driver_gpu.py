"""calcMG_loop_wOneD_TSM_EvenOdd with the loop output on (qudaAmdSetLoopOutput), through the committed consumer
tests/consumer/loop_driver.cpp: 8^4, one multigrid hierarchy, the sink registered.  (a) Nstoch = 4, Ndump = 2, lockstep on and off,
both mass normalisations; (b) the truncated solver method with TSM_NLP = 4, NdumpLP = 2, TSM_NHP = 2, NdumpHP = 1.  The files must
carry the reference's names (lib/interface_quda.cpp:9060-9410), line counts and line formats (writeLoops_ASCII,
lib/qudaQKXTM_Loops_Kepler.cpp:501-575), and every value must equal the running sum of qudaAmdContractLoop over the solutions the
sink captured (divided by the sink's 2 kappa where it applied, times 0.25 for the one-derivative types) to 1e-12 relative to the
block maximum; dump NNNN is the sum of the first NNNN vectors.  With the output off the same run writes no file and the sink sees
the same solutions."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from synth import smooth_gauge  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "quda-qkxtm-multigrid_amd", "lib")
X = (8, 8, 8, 8)
KAPPA, QSQ = 0.124, 2
TYPES = ["Scalar", "dOp", "Loops", "LoopsCv", "LpsDw", "LpsDwCv"]
FIRST = {"Scalar": 0, "dOp": 1, "Loops": 2, "LoopsCv": 6, "LpsDw": 10, "LpsDwCv": 14}
_F = r"([+-]\d\.\d{15}e[+-]\d{2,3})"
ULOCAL_LINE = re.compile(r"(\d{2}) (\d{2}) ([+-]\d+) ([+-]\d+) ([+-]\d+) %s %s\n" % (_F, _F))
ONED_LINE = re.compile(r"(\d{2}) (\d{2}) (\d{2}) ([+-]\d+) ([+-]\d+) ([+-]\d+) %s %s\n" % (_F, _F))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("loop_driver")
    exe = str(d / "loop_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", INC, "-I", "/opt/rocm/include",
                    os.path.join(ROOT, "tests", "consumer", "loop_driver.cpp"), "-o", exe, "-L" + LIBDIR, "-lquda", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True, text=True)
    gauge = smooth_gauge(X, 0.35)
    gfile = d / "gauge.bin"
    np.ascontiguousarray(gauge).tofile(str(gfile))
    return exe, str(gfile), gauge


@pytest.fixture(scope="module")
def qa_loop():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


def _run(driver, outdir, output, massnorm, lockstep, tsm):
    exe, gfile, _ = driver
    prefix = os.path.join(str(outdir), "run")
    env = dict(os.environ, QUDA_AMD_QKXTM_LOCKSTEP="1" if lockstep else "0")
    r = subprocess.run([exe, gfile] + [str(v) for v in X] + [prefix, str(int(output)), str(int(massnorm)), str(int(tsm))], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return prefix


def _read_sink(path):
    sols = {}
    raw = open(path, "rb").read()
    o = 0
    while o < len(raw):
        kind = raw[o:o + 16].split(b"\0")[0].decode()
        index, flavor, has_src, nreal = np.frombuffer(raw, dtype=np.int32, count=4, offset=o + 16)
        o += 32 + (nreal * 8 if has_src else 0)
        sols[(kind, int(index))] = np.frombuffer(raw, dtype=np.float64, count=nreal, offset=o).copy()
        o += nreal * 8
    assert nreal == int(np.prod(X)) * 24
    return sols


def _check_file(path, typ, want, moms):
    """want: (18, T, Nmoms, 16) running sum; lines run momentum, t, gm, and for the one-derivative types mu outermost (appended)"""
    lines = open(path).readlines()
    Nm, T = len(moms), X[3]
    oned = typ not in ("Scalar", "dOp")
    assert len(lines) == Nm * T * 16 * (4 if oned else 1), (path, len(lines))
    k = 0
    worst = 0.0
    for mu in range(4 if oned else 1):
        blk = (0.25 if oned else 1.0) * want[FIRST[typ] + mu]
        bmax = np.max(np.abs(blk))
        for ip in range(Nm):
            for t in range(T):
                for gm in range(16):
                    g = (ONED_LINE if oned else ULOCAL_LINE).fullmatch(lines[k])
                    assert g, (path, lines[k])
                    k += 1
                    ints = [int(v) for v in g.groups()[:-2]]
                    assert ints == ([t, gm, mu] if oned else [t, gm]) + moms[ip].tolist(), (path, lines[k - 1])
                    got = complex(float(g.groups()[-2]), float(g.groups()[-1]))
                    worst = max(worst, abs(got - blk[t, ip, gm]) / bmax)
    print("%s: worst deviation %.3e of the block maximum" % (os.path.basename(path), worst))
    assert worst < 1e-12, (path, worst)


def _running_sums(qa, ip, sols, kind, n, scale):
    out, acc = [], 0
    for i in range(n):
        acc = acc + qa.contract_loop(sols[(kind, i)] * scale, ip, QSQ, X[:3])
        out.append(acc)
    return out


def _setup(qa, driver):
    _, _, gauge = driver
    qa.load_gauge(gauge, qa.gauge_param(X, t_boundary=qa.QUDA_PERIODIC_T))
    return qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, KAPPA, 0.005, +1, "ee", 0, cuda_prec=8, solution_type=qa.QUDA_MAT_SOLUTION,
                           gamma_basis=qa.QUDA_UKQCD_GAMMA_BASIS)


def _loop_files(outdir):
    return sorted(f for f in os.listdir(str(outdir)) if ".loop." in f)


@pytest.mark.parametrize("massnorm,lockstep", [(0, True), (1, False), (1, True), (0, False)])
def test_plain_run_writes_the_reference_files(qa_loop, driver, tmp_path, massnorm, lockstep):
    qa = qa_loop
    prefix = _run(driver, tmp_path, True, massnorm, lockstep, False)
    ip = _setup(qa, driver)
    sols = _read_sink(prefix + ".sink")
    assert sorted(sols) == [("loop_stoch", i) for i in range(4)]
    want_names = sorted("run_loop_stoch_MG_%s.loop.%04d.1_0" % (t, n) for t in TYPES for n in (2, 4))
    assert _loop_files(tmp_path) == want_names
    moms = qa.loop_momenta(X[:3], QSQ)
    sums = _running_sums(qa, ip, sols, "loop_stoch", 4, 1.0 / (2.0 * KAPPA) if massnorm else 1.0)
    for n in (2, 4):
        for t in TYPES:
            _check_file(os.path.join(str(tmp_path), "run_loop_stoch_MG_%s.loop.%04d.1_0" % (t, n)), t, sums[n - 1], moms)
    assert all(np.max(np.abs(sums[3][k])) > 0 for k in range(18))


def test_tsm_run_writes_the_three_families(qa_loop, driver, tmp_path):
    qa = qa_loop
    prefix = _run(driver, tmp_path, True, 0, True, True)
    ip = _setup(qa, driver)
    sols = _read_sink(prefix + ".sink")
    assert sorted(sols) == sorted([("loop_LP", i) for i in range(4)] + [("loop_HP", i) for i in range(2)] + [("loop_HP_LP", i) for i in range(2)])
    fam = [("run_loop_stoch_TSM_MG_NLP%04d_%s.loop.1_0", "loop_LP", (2, 4)), ("run_loop_stoch_TSM_MG_HighPrec_NHP%04d_%s.loop.1_0", "loop_HP", (1, 2)),
           ("run_loop_stoch_TSM_MG_LowPrec_NHP%04d_%s.loop.1_0", "loop_HP_LP", (1, 2))]
    assert _loop_files(tmp_path) == sorted(pat % (n, t) for pat, _, dumps in fam for n in dumps for t in TYPES)
    moms = qa.loop_momenta(X[:3], QSQ)
    for pat, kind, dumps in fam:
        sums = _running_sums(qa, ip, sols, kind, max(dumps), 1.0)
        for n in dumps:
            for t in TYPES:
                _check_file(os.path.join(str(tmp_path), pat % (n, t)), t, sums[n - 1], moms)


def test_output_off_writes_no_file_and_solves_the_same(driver, tmp_path):
    on, off = tmp_path / "on", tmp_path / "off"
    on.mkdir(); off.mkdir()
    a = _read_sink(_run(driver, on, True, 0, True, False) + ".sink")
    b = _read_sink(_run(driver, off, False, 0, True, False) + ".sink")
    assert _loop_files(off) == [] and len(_loop_files(on)) == 12
    assert sorted(a) == sorted(b)
    for key in a:
        # the contraction reads the solution and changes nothing the solver sees: same sources, same solves
        dev = np.max(np.abs(a[key] - b[key])) / np.max(np.abs(a[key]))
        print(key, "relative deviation between the runs %.3e" % dev)
        assert dev == 0.0, (key, dev)
