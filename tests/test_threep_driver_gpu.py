"""calcMG_threepTwop_EvenOdd with the three-point output on (qudaAmdSetThreepOutput), through the committed consumer
tests/consumer/threep_driver.cpp: 8^4, two source positions of which only the first has run3pt_src = 1, sink separations 2 (one
projector, G5G123) and 4 (two projectors, G4 and G5G2; 4 + t0 = 9 wraps), the proton, mass normalisation (the 2 kappa rescale), up /
down multigrid hierarchies, the links of the derivative given by the caller, the sink registered.  The files must carry the
reference's names, line counts and line formats (writeThrp_ASCII, lib/qudaQKXTM_Contraction_Kepler.cpp:2842-3003) and the numbers
qudaAmdContractThreep computes from the seq_part* and prop_* solutions the sink captured, to the %+e rounding (the closeness rule of
tests/test_twop_driver_gpu.py).  The seq_part* sink calls come in the order (its, ip, part, column) with the index
((isource * Ntsink + its) * Nproj[its] + ip) * 12 + column and the flavour of the solve; every captured sequential solution
reproduces its captured source under the oracle's tm_mat at that twist (5e-10 for the solver's 1e-10 on the even-odd system, the
bound of tests/test_qkxtm_gpu.py for the forward solves).  The one-by-one order (QUDA_AMD_QKXTM_LOCKSTEP=0) writes the same files;
with the output off the run writes no file and makes no seq_part* call."""
import importlib
import os
import re
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

from synth import smooth_gauge  # noqa: E402
from test_twop_gpu import _lex_gauge  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "quda-qkxtm-multigrid_amd", "lib")
X = (8, 8, 8, 8)
SOURCES = [(1, 2, 3, 5), (6, 3, 1, 7)]   # only the first runs the three-point stage
KAPPA, MU = 0.124, 0.005
QSQ = 2
TSINK, NPROJ, PROJ_LIST = [2, 4], [1, 2], [["G5G123"], ["G4", "G5G2"]]
STEPS = [(its, ip) for its in range(2) for ip in range(NPROJ[its])]
_F = r"([+-]\d\.\d{6}e[+-]\d{2,3})"
_M = r"([+-]\d+) ([+-]\d+) ([+-]\d+)"
LINE2 = re.compile(r"(\d+) \t (\d+) \t %s \t %s %s\n" % (_M, _F, _F))              # ultra_local: iop, it; noether: dir, it
LINE3 = re.compile(r"(\d+) \t (\d+) \t (\d+) \t %s \t %s %s\n" % (_M, _F, _F))     # oneD: iop, dir, it


@pytest.fixture(scope="module")
def qa():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()


@pytest.fixture(scope="module")
def driver(tmp_path_factory, oracle):
    d = tmp_path_factory.mktemp("threep_driver")
    exe = str(d / "threep_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", INC, "-I", "/opt/rocm/include",
                    os.path.join(ROOT, "tests", "consumer", "threep_driver.cpp"), "-o", exe, "-L" + LIBDIR, "-lquda", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True, text=True)
    gauge = smooth_gauge(X, 0.35)
    g_lex = _lex_gauge(oracle, gauge, X)
    np.ascontiguousarray(gauge).tofile(str(d / "gauge.bin"))
    np.ascontiguousarray(g_lex).tofile(str(d / "gauge_lex.bin"))
    return exe, str(d / "gauge.bin"), str(d / "gauge_lex.bin"), gauge, g_lex


def _run(driver, outdir, output, lockstep):
    exe, gfile, lfile = driver[:3]
    os.makedirs(str(outdir), exist_ok=True)
    prefix = os.path.join(str(outdir), "run")
    env = dict(os.environ, QUDA_AMD_QKXTM_LOCKSTEP="1" if lockstep else "0")
    r = subprocess.run([exe, gfile, lfile] + [str(v) for v in X] + [prefix, str(int(output)), "1"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return prefix


def _read_sink(path):
    """the records in the order of the calls: (kind, index, flavour, source or None, solution)"""
    recs = []
    raw = open(path, "rb").read()
    o = 0
    while o < len(raw):
        kind = raw[o:o + 16].split(b"\0")[0].decode()
        index, flavor, has_src, nreal = (int(v) for v in np.frombuffer(raw, dtype=np.int32, count=4, offset=o + 16))
        o += 32
        src = None
        if has_src:
            src = np.frombuffer(raw, dtype=np.float64, count=nreal, offset=o)
            o += nreal * 8
        recs.append((kind, index, flavor, src, np.frombuffer(raw, dtype=np.float64, count=nreal, offset=o)))
        o += nreal * 8
    return recs


def _names(s):
    out = {}
    for its, ip in STEPS:
        for part, flavor in ((1, "up"), (2, "down")):   # proton: part 1 inserts on the up quark
            for typ in ("ultra_local", "noether", "oneD"):
                out[(its, ip, part, typ)] = "run.threep_tsink%d_proj%s.proton.%s.%s.SS.%02d.%02d.%02d.%02d.dat" % ((TSINK[its], PROJ_LIST[its][ip], flavor, typ) + s)
    return out


def _parse(path, pattern, nidx, moms, T):
    """every line against its format; returns the values in file order, shape (..., T, Nm) complex, after checking the running indices"""
    lines = open(path).readlines()
    Nm = len(moms)
    heads, vals = [], []
    for ln in lines:
        g = pattern.fullmatch(ln)
        assert g, (path, ln)
        heads.append([int(v) for v in g.groups()[:nidx + 3]])
        vals.append(complex(float(g.group(nidx + 4)), float(g.group(nidx + 5))))
    return np.array(heads), np.array(vals), len(lines), Nm * T


def _close(got, want, blockmax):
    """the rule of the two-point driver test, on the real and the imaginary parts: the %+e rounding, and 1e-12 of the block's largest entry"""
    g, w = np.stack([got.real, got.imag]), np.stack([want.real, want.imag])
    return np.all(np.abs(g - w) <= 2e-6 * np.abs(w) + 1e-12 * blockmax)


def _file_arrays(prefix_dir, s, moms, T):
    """(its, ip, part) -> local (16, T, Nm), noether (4, T, Nm), oneD (16, 4, T, Nm) as written, with counts, formats and indices checked"""
    Nm = len(moms)
    names = _names(s)
    got = sorted(f for f in os.listdir(prefix_dir) if ".threep" in f)
    assert got == sorted(names.values())
    out = {}
    mom_cols = np.asarray(moms)
    for its, ip in STEPS:
        for part in (1, 2):
            arrs = []
            for typ, pattern, lead in (("ultra_local", LINE2, (16,)), ("noether", LINE2, (4,)), ("oneD", LINE3, (16, 4))):
                heads, vals, n, _ = _parse(os.path.join(prefix_dir, names[(its, ip, part, typ)]), pattern, len(lead) + 1, moms, T)
                shape = lead + (T, Nm)
                assert n == int(np.prod(shape)), (typ, n)
                want_heads = np.stack(np.meshgrid(*[np.arange(k) for k in shape], indexing="ij"), axis=-1).reshape(-1, len(shape))
                assert np.array_equal(heads[:, :len(shape) - 1], want_heads[:, :-1])          # iop / dir / it run in the order of writeThrp_ASCII
                assert np.array_equal(heads[:, len(shape) - 1:], mom_cols[want_heads[:, -1]])   # the momentum of the line
                arrs.append(vals.reshape(shape))
            out[(its, ip, part)] = arrs
    return out


@pytest.fixture(scope="module")
def lockstep_run(driver, tmp_path_factory):
    d = tmp_path_factory.mktemp("threep_lockstep")
    prefix = _run(driver, d, True, True)
    return str(d), _read_sink(prefix + ".sink")


def _seq_records(recs):
    return [r for r in recs if r[0].startswith("seq_part")]


def test_sink_calls_and_residuals(lockstep_run, driver, oracle):
    _, recs = lockstep_run
    gauge = driver[3]
    assert sum(r[0] == "prop_up" for r in recs) == 24 and sum(r[0] == "prop_dn" for r in recs) == 24
    seq = _seq_records(recs)
    want = [("seq_part%d" % part, ((0 * 2 + its) * NPROJ[its] + ip) * 12 + col, -1 if part == 1 else +1)
            for its, ip in STEPS for part in (1, 2) for col in range(12)]
    assert [r[:3] for r in seq] == want
    # the sequential solves of the only three-point source come after its 24 forward solves and before those of the next source
    kinds = [r[0] for r in recs]
    first = kinds.index("seq_part1")
    assert set(kinds[:first]) == {"prop_up", "prop_dn"} and first == 24 and not any(k.startswith("seq") for k in kinds[first + 72:])
    assert sorted(r[1] for r in recs[first + 72:]) == sorted(list(range(12, 24)) * 2)
    oracle.set_threads(8)
    try:
        worst = 0.0
        for kind, index, flavor, src, sol in seq:
            assert src is not None and np.linalg.norm(src) > 0
            b = oracle.lex_to_eo(oracle.ukqcd_to_dr(src.reshape(-1, 24)).reshape(-1), list(X), 24)
            x = oracle.lex_to_eo(oracle.ukqcd_to_dr(sol.reshape(-1, 24)).reshape(-1), list(X), 24) / (2 * KAPPA)   # mass normalisation
            worst = max(worst, float(np.linalg.norm(b - oracle.tm_mat(gauge, x, list(X), KAPPA, MU, flavor, 0)) / np.linalg.norm(b)))
    finally:
        oracle.set_threads(1)
    print("worst residual of the 72 sequential solutions under tm_mat: %.3e" % worst)
    assert worst < 5e-10, worst


def test_driver_writes_the_reference_files(qa, lockstep_run, driver):
    outdir, recs = lockstep_run
    gauge, g_lex = driver[3], driver[4]
    qa.load_gauge(gauge, qa.gauge_param(X, t_boundary=qa.QUDA_PERIODIC_T))
    moms = qa.twop_momenta(QSQ)
    T = X[3]
    s = SOURCES[0]
    files = _file_arrays(outdir, s, moms, T)
    props = {(k, i): sol for k, i, _, _, sol in recs if k.startswith("prop")}
    fwd = {+1: np.stack([props[("prop_up", c)] for c in range(12)]), -1: np.stack([props[("prop_dn", c)] for c in range(12)])}
    seq = _seq_records(recs)
    n = 0
    for its, ip in STEPS:
        for part in (1, 2):
            sols = np.stack([r[4] for r in seq[n:n + 12]])
            n += 12
            loc, noe, one = qa.contract_threep(sols, fwd[+1 if part == 1 else -1], g_lex, s, QSQ, TSINK[its], qa.PROTON, part)
            assert np.max(np.abs(loc)) > 0 and np.max(np.abs(noe)) > 0 and np.max(np.abs(one)) > 0
            got = files[(its, ip, part)]
            want = [loc.transpose(2, 0, 1), noe.transpose(2, 0, 1), one.transpose(3, 2, 0, 1)]   # the files' loop orders
            for typ, g, w in zip(("ultra_local", "noether", "oneD"), got, want):
                lead = w.shape[:-2]
                for blk in np.ndindex(*lead):
                    assert _close(g[blk], w[blk], np.max(np.abs(w[blk]))), (its, ip, part, typ, blk, np.max(np.abs(g[blk] - w[blk])), np.max(np.abs(w[blk])))


def test_one_by_one_order_writes_the_same_files(qa, lockstep_run, driver, tmp_path):
    """the two orders solve the same systems to 1e-10; the correlators are bilinear in solutions whose errors the inverse operator
    amplifies by at most 1 / (2 kappa mu) ~ 1e3, so they agree to 1e-6 of a block's largest entry on top of the %+e rounding"""
    outdir, recs = lockstep_run
    prefix = _run(driver, tmp_path / "one", True, False)
    moms = qa.twop_momenta(QSQ)
    a, b = _file_arrays(outdir, SOURCES[0], moms, X[3]), _file_arrays(str(tmp_path / "one"), SOURCES[0], moms, X[3])
    assert [r[:3] for r in _seq_records(_read_sink(prefix + ".sink"))] == [r[:3] for r in _seq_records(recs)]
    for key in a:
        for g, w in zip(b[key], a[key]):
            for blk in np.ndindex(*w.shape[:-2]):
                assert np.all(np.abs(g[blk] - w[blk]) <= 2e-6 * np.abs(w[blk]) + 1e-6 * np.max(np.abs(w[blk]))), (key, blk)


def test_driver_with_output_off_writes_no_file_and_makes_no_sink_call(driver, tmp_path):
    prefix = _run(driver, tmp_path, False, True)
    assert not [f for f in os.listdir(str(tmp_path)) if ".threep" in f or ".twop." in f]
    kinds = [r[0] for r in _read_sink(prefix + ".sink")]
    assert len(kinds) == 48 and not any(k.startswith("seq") for k in kinds)
