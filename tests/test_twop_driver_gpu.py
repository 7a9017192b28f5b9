"""calcMG_threepTwop_EvenOdd with the two-point output on (qudaAmdSetTwopOutput), through the committed consumer
tests/consumer/twop_driver.cpp: 8^4, two source positions (one whose t0 makes t wrap), up / down multigrid hierarchies, the sink
registered.  The files must carry the reference's names (lib/interface_quda.cpp:6351-6363), line counts and line formats
(lib/qudaQKXTM_Contraction_Kepler.cpp:849-905, :1563-1590), and the numbers qudaAmdContractTwop computes from the propagators
the sink captured, to the %+e rounding.  Both solve orders (lockstep multi-source and one by one) and both normalisations (the
2 kappa rescale) go through the device-resident path; with the output off the same run writes no file."""
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
SOURCES = [(1, 2, 3, 5), (6, 3, 1, 7)]
QSQ, NSMEAR, ALPHA = 2, 2, 0.5
_F = r"([+-]\d\.\d{6}e[+-]\d{2,3})"
MESON_LINE = re.compile(r"(\d+) \t (\d+) \t ([+-]\d+) ([+-]\d+) ([+-]\d+) \t %s %s \t %s %s\n" % (_F, _F, _F, _F))
BARYON_LINE = re.compile(r"(\d+) \t (\d+) \t ([+-]\d+) ([+-]\d+) ([+-]\d+) \t (\d) (\d) \t %s %s \t %s %s\n" % (_F, _F, _F, _F))


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    d = tmp_path_factory.mktemp("twop_driver")
    exe = str(d / "twop_driver")
    subprocess.run(["g++", "-std=c++17", "-O1", "-D__HIP_PLATFORM_AMD__", "-I", INC, "-I", "/opt/rocm/include",
                    os.path.join(ROOT, "tests", "consumer", "twop_driver.cpp"), "-o", exe, "-L" + LIBDIR, "-lquda", "-L/opt/rocm/lib", "-lamdhip64",
                    "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"], check=True, capture_output=True, text=True)
    gauge = smooth_gauge(X, 0.35)
    gfile = d / "gauge.bin"
    np.ascontiguousarray(gauge).tofile(str(gfile))
    return exe, str(gfile), gauge


def _run(driver, outdir, output, massnorm, lockstep):
    exe, gfile, _ = driver
    prefix = os.path.join(str(outdir), "run")
    env = dict(os.environ, QUDA_AMD_QKXTM_LOCKSTEP="1" if lockstep else "0")
    r = subprocess.run([exe, gfile] + [str(v) for v in X] + [prefix, str(int(output)), str(int(massnorm))], capture_output=True, text=True,
                       timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return prefix


def _read_sink(path):
    V = int(np.prod(X))
    props = {}
    raw = open(path, "rb").read()
    o = 0
    while o < len(raw):
        kind = raw[o:o + 16].split(b"\0")[0].decode()
        index, flavor, has_src, nreal = np.frombuffer(raw, dtype=np.int32, count=4, offset=o + 16)
        o += 32 + (nreal * 8 if has_src else 0)
        props[(kind, int(index), int(flavor))] = np.frombuffer(raw, dtype=np.float64, count=nreal, offset=o).copy()
        o += nreal * 8
    assert nreal == V * 24
    return props


def _close(got, want, blockmax):
    return np.all(np.abs(got - want) <= 2e-6 * np.abs(want) + 1e-12 * blockmax)


@pytest.mark.parametrize("massnorm,lockstep", [(0, True), (1, False)])
def test_driver_writes_the_reference_files(qa_twop, driver, tmp_path, massnorm, lockstep):
    qa = qa_twop
    prefix = _run(driver, tmp_path, True, massnorm, lockstep)
    _, _, gauge = driver
    V = int(np.prod(X))
    qa.load_gauge(gauge, qa.gauge_param(X, t_boundary=qa.QUDA_PERIODIC_T))
    ape = np.fromfile(prefix + ".ape").reshape(4, V * 18)
    props = _read_sink(prefix + ".sink")
    assert len(props) == 48
    moms = qa.twop_momenta(QSQ)
    Nm, T = len(moms), X[3]
    names = sorted(f for f in os.listdir(str(tmp_path)) if ".twop." in f)
    want_names = sorted("run.twop.%s.SS.%02d.%02d.%02d.%02d.dat" % ((kind,) + s) for kind in ("mesons", "baryons") for s in SOURCES)
    assert names == want_names
    for isrc, s in enumerate(SOURCES):
        up = np.stack([props[("prop_up", 12 * isrc + isc, 1)] for isc in range(12)])
        dn = np.stack([props[("prop_dn", 12 * isrc + isc, -1)] for isc in range(12)])
        mes, bar = qa.contract_twop(up, dn, ape, s, QSQ, NSMEAR, ALPHA)
        lines = open(prefix + ".twop.mesons.SS.%02d.%02d.%02d.%02d.dat" % s).readlines()
        assert len(lines) == 10 * T * Nm
        k = 0
        for ip in range(10):
            blk = np.max(np.abs(mes[:, :, :, ip]))
            for it in range(T):
                for m in range(Nm):
                    g = MESON_LINE.fullmatch(lines[k])
                    assert g, lines[k]
                    k += 1
                    assert [int(v) for v in g.groups()[:5]] == [ip, it] + moms[m].tolist()
                    vals = np.array([float(v) for v in g.groups()[5:]])
                    want = np.array([mes[it, m, 0, ip].real, mes[it, m, 0, ip].imag, mes[it, m, 1, ip].real, mes[it, m, 1, ip].imag])
                    assert _close(vals, want, blk), (lines[k - 1], want)
        lines = open(prefix + ".twop.baryons.SS.%02d.%02d.%02d.%02d.dat" % s).readlines()
        assert len(lines) == 16 * 10 * T * Nm
        k = 0
        for ip in range(10):
            blk = np.max(np.abs(bar[:, :, :, ip]))
            for it in range(T):
                for m in range(Nm):
                    for ga in range(4):
                        for gb in range(4):
                            g = BARYON_LINE.fullmatch(lines[k])
                            assert g, lines[k]
                            k += 1
                            assert [int(v) for v in g.groups()[:7]] == [ip, it] + moms[m].tolist() + [ga, gb]
                            vals = np.array([float(v) for v in g.groups()[7:]])
                            w0, w1 = bar[it, m, 0, ip, ga, gb], bar[it, m, 1, ip, ga, gb]
                            assert _close(vals, np.array([w0.real, w0.imag, w1.real, w1.imag]), blk), (lines[k - 1], w0, w1)
        assert np.max(np.abs(mes)) > 0 and np.max(np.abs(bar)) > 0


def test_driver_with_output_off_writes_no_file(driver, tmp_path):
    _run(driver, tmp_path, False, 0, True)
    assert not [f for f in os.listdir(str(tmp_path)) if ".twop." in f or ".threep" in f]


@pytest.fixture(scope="module")
def qa_twop():
    mod = importlib.import_module("quda-qkxtm-multigrid_amd")
    mod.init(0)
    yield mod
    mod.end()
