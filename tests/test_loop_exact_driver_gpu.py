"""calcMG_loop_wOneD_TSM_wExact with exact deflation, through the committed consumer tests/consumer/loop_exact_driver.cpp: 8^4, the
hierarchy and gauge field of loop_driver.cpp, nEv = 12, nKv = 32, Chebyshev degree 20 on [0.2, 4.0], tol 1e-10, deflation steps {4, 12},
Nstoch = 4, Ndump = 2.  (A numpy prototype of the eigensolver on the oracle's operator found the twelve modes 0.0208 .. 0.0218 in 4 cycles.)

(a) output on: exactly the files <prefix>_exact_NeV{4,12}_<type>.loop.1_0 and <prefix>_stoch_NeV{4,12}_<type>.loop.{0002,0004}.1_0; the
exact values equal sum_i contract_loop(v_i) / lambda_i over the "eigvec" vectors the sink received and the eigenvalues
qudaAmdLastEigenvalues reports, the stochastic values the running sum of contract_loop over the sink's solutions projected in numpy
with the first n of those vectors; both to 1e-12 of the block maximum, in the reference's line format.  (b) the truncated solver method
(TSM_NLP = 4, NdumpLP = 2, TSM_NHP = 2, NdumpHP = 1): the names <prefix>_stoch_TSM_NeV<n>_...; the NLP family of n = 12 by value.
(c) output off: no file, the same solutions bit for bit.  (d) isFullOp = false and deflStep = {13} exit non-zero and name the field."""
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
STEPS = (4, 12)
TYPES = ["Scalar", "dOp", "Loops", "LoopsCv", "LpsDw", "LpsDwCv"]
FIRST = {"Scalar": 0, "dOp": 1, "Loops": 2, "LoopsCv": 6, "LpsDw": 10, "LpsDwCv": 14}
_F = r"([+-]\d\.\d{15}e[+-]\d{2,3})"
ULOCAL_LINE = re.compile(r"(\d{2}) (\d{2}) ([+-]\d+) ([+-]\d+) ([+-]\d+) %s %s\n" % (_F, _F))
ONED_LINE = re.compile(r"(\d{2}) (\d{2}) (\d{2}) ([+-]\d+) ([+-]\d+) ([+-]\d+) %s %s\n" % (_F, _F))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("loop_exact_driver")
    exe = str(d / "loop_exact_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", INC, "-I", "/opt/rocm/include",
                    os.path.join(ROOT, "tests", "consumer", "loop_exact_driver.cpp"), "-o", exe, "-L" + LIBDIR, "-lquda", "-L/opt/rocm/lib", "-lamdhip64",
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


def _launch(driver, outdir, output, tsm, bad=0):
    exe, gfile, _ = driver
    prefix = os.path.join(str(outdir), "run")
    r = subprocess.run([exe, gfile] + [str(v) for v in X] + [prefix, str(int(output)), str(int(tsm)), str(int(bad))], capture_output=True, text=True, timeout=600)
    return prefix, r


def _run(driver, outdir, output, tsm):
    prefix, r = _launch(driver, outdir, output, tsm)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return prefix


@pytest.fixture(scope="module")
def plain_on(driver, tmp_path_factory):
    d = tmp_path_factory.mktemp("plain_on")
    return d, _run(driver, d, True, False)


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
    """want: (18, T, Nmoms, 16) sum; lines run momentum, t, gm, and for the one-derivative types mu outermost (appended)"""
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


def _setup(qa, driver):
    _, _, gauge = driver
    qa.load_gauge(gauge, qa.gauge_param(X, t_boundary=qa.QUDA_PERIODIC_T))
    return qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, KAPPA, 0.005, +1, "ee", 0, cuda_prec=8, solution_type=qa.QUDA_MAT_SOLUTION,
                           gamma_basis=qa.QUDA_UKQCD_GAMMA_BASIS)


def _loop_files(outdir):
    return sorted(f for f in os.listdir(str(outdir)) if ".loop." in f)


def _cplx(v):
    return v[0::2] + 1j * v[1::2]


def _eigvecs(sols):
    U = np.stack([_cplx(sols[("eigvec", i)]) for i in range(12)])
    orth = np.max(np.abs(U.conj() @ U.T - np.eye(12)))
    print("|U^+ U - 1| of the sink's eigenvectors: %.3e" % orth)
    assert orth <= 1e-12
    return U


def _projected(x, U, n):
    xc = _cplx(x)
    p = xc - U[:n].T @ (U[:n].conj() @ xc)
    return np.ascontiguousarray(np.stack([p.real, p.imag], axis=-1).reshape(-1))


def _running_sums(qa, ip, sols, kind, count, U, n):
    out, acc = [], 0
    for i in range(count):
        acc = acc + qa.contract_loop(_projected(sols[(kind, i)], U, n), ip, QSQ, X[:3])
        out.append(acc)
    return out


def _exact_names():
    return ["run_loop_exact_NeV%d_%s.loop.1_0" % (n, t) for n in STEPS for t in TYPES]


def test_plain_run_writes_the_exact_and_the_stochastic_part(qa_loop, driver, plain_on):
    qa = qa_loop
    outdir, prefix = plain_on
    ip = _setup(qa, driver)
    sols = _read_sink(prefix + ".sink")
    assert sorted(sols) == sorted([("eigvec", i) for i in range(12)] + [("loop_stoch", i) for i in range(4)])
    evals = np.fromfile(prefix + ".evals")
    print("eigenvalues:", evals)
    assert len(evals) == 12 and np.all(np.diff(evals) >= 0) and evals[0] >= (2 * KAPPA * 0.005) ** 2
    want_names = sorted(_exact_names() + ["run_loop_stoch_NeV%d_%s.loop.%04d.1_0" % (n, t, d) for n in STEPS for t in TYPES for d in (2, 4)])
    assert _loop_files(outdir) == want_names
    moms = qa.loop_momenta(X[:3], QSQ)
    U = _eigvecs(sols)
    exact, done = 0, 0
    for n in STEPS:
        for i in range(done, n):
            exact = exact + qa.contract_loop(sols[("eigvec", i)], ip, QSQ, X[:3]) / evals[i]
        done = n
        for t in TYPES:
            _check_file(os.path.join(str(outdir), "run_loop_exact_NeV%d_%s.loop.1_0" % (n, t)), t, exact, moms)
        sums = _running_sums(qa, ip, sols, "loop_stoch", 4, U, n)
        for d in (2, 4):
            for t in TYPES:
                _check_file(os.path.join(str(outdir), "run_loop_stoch_NeV%d_%s.loop.%04d.1_0" % (n, t, d)), t, sums[d - 1], moms)
        assert all(np.max(np.abs(sums[3][k])) > 0 for k in range(18))


def test_tsm_run_writes_the_deflated_families(qa_loop, driver, tmp_path):
    qa = qa_loop
    prefix = _run(driver, tmp_path, True, True)
    ip = _setup(qa, driver)
    sols = _read_sink(prefix + ".sink")
    assert sorted(sols) == sorted([("eigvec", i) for i in range(12)] + [("loop_LP", i) for i in range(4)] + [("loop_HP", i) for i in range(2)] + [("loop_HP_LP", i) for i in range(2)])
    fam = [("run_loop_stoch_TSM_NeV%d_NLP%04d_%s.loop.1_0", (2, 4)), ("run_loop_stoch_TSM_NeV%d_HighPrec_NHP%04d_%s.loop.1_0", (1, 2)),
           ("run_loop_stoch_TSM_NeV%d_LowPrec_NHP%04d_%s.loop.1_0", (1, 2))]
    assert _loop_files(tmp_path) == sorted(_exact_names() + [pat % (n, d, t) for pat, dumps in fam for n in STEPS for d in dumps for t in TYPES])
    moms = qa.loop_momenta(X[:3], QSQ)
    U = _eigvecs(sols)
    sums = _running_sums(qa, ip, sols, "loop_LP", 4, U, 12)
    for d in (2, 4):
        for t in TYPES:
            _check_file(os.path.join(str(tmp_path), fam[0][0] % (12, d, t)), t, sums[d - 1], moms)


def test_output_off_writes_no_file_and_solves_the_same(driver, plain_on, tmp_path):
    outdir, prefix = plain_on
    a = _read_sink(prefix + ".sink")
    b = _read_sink(_run(driver, tmp_path, False, False) + ".sink")
    assert _loop_files(tmp_path) == [] and len(_loop_files(outdir)) == 36
    assert sorted(a) == sorted(b)
    for key in a:
        dev = np.max(np.abs(a[key] - b[key])) / np.max(np.abs(a[key]))
        print(key, "relative deviation between the runs %.3e" % dev)
        assert dev == 0.0, (key, dev)


@pytest.mark.parametrize("bad,field", [(1, "isFullOp"), (2, "deflStep")])
def test_bad_parameters_stop_with_the_field_name(driver, tmp_path, bad, field):
    _, r = _launch(driver, tmp_path, True, False, bad)
    print((r.stdout + r.stderr)[-600:])
    assert r.returncode != 0
    assert field in r.stdout + r.stderr
    assert _loop_files(tmp_path) == []
