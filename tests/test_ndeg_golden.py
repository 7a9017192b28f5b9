"""Host reference of the non-degenerate twisted-mass doublet, and its check against the reference's own host operators.

The doublet operators are composed here in numpy from the oracle's single-flavour hop (oracle.wil_dslash) and the flavour twist
    out1 = d (in1 + i a g5 in1 + b in2)        out2 = d (in2 - i a g5 in2 + b in1)
with a = 2 kappa mu, b = -2 kappa epsilon, d = 1 (direct) or a = -2 kappa mu, b = +2 kappa epsilon, d = 1 / (1 + a^2 - b^2) (inverse);
dagger flips the sign of a.  A parity doublet is [flavour 1: Vh 24][flavour 2: Vh 24], a full doublet [even doublet][odd doublet].

tests/golden/ndeg_<dims>.p*.npz hold what the reference's tm_ndeg_dslash / tm_ndeg_matpc / tm_ndeg_mat give for kappa = 0.12, mu = 0.3,
epsilon = 0.2 on the committed gauge field and `spinor2` (tools/ndeg_golden/).  The composition reproduces all 26 outputs bit for bit on
both lattices (maximum difference 0.0): the arithmetic is written in the reference's order of operations.  The files are split into parts
(.p0, .p1, ...) to keep every committed file below 1 MiB.

The GPU tests import ndeg_dslash / ndeg_matpc / ndeg_mat / ndeg_twist and load_golden from here."""
import glob
import os

import numpy as np
import pytest

import qa_cases as qc

MPC = ("ee", "oo", "eeasym", "ooasym")
LATTICES = ((4, 4, 4, 4), (6, 4, 2, 8))
_G5 = np.array([1.0, 1.0, -1.0, -1.0]).reshape(1, 4, 1)


def load_golden(X):
    """(dict of the ndeg arrays and parameters, gauge (4, V 18), committed spinor) of one golden lattice"""
    tag = "%dx%dx%dx%d" % tuple(X)
    parts = sorted(glob.glob(os.path.join(qc.GOLD, "ndeg_%s.p*.npz" % tag)))
    assert parts, "no doublet goldens for %s" % tag
    z = {}
    for p in parts:
        with np.load(p) as f:
            z.update({k: f[k] for k in f.files})
    base = np.load(os.path.join(qc.GOLD, "ref_%s.npz" % tag))
    gauge = np.stack([base["gauge%d" % d] for d in range(4)])
    return z, gauge, base["spinor"]


def case_names(z):
    return sorted(k for k in z if k.startswith("ndeg_"))


def ndeg_twist(v, kappa, mu, epsilon, dagger, inverse):
    """the flavour twist on a parity doublet (or any [flavour 1][flavour 2] array)"""
    if inverse:
        a, b = -2.0 * kappa * mu, 2.0 * kappa * epsilon
        d = 1.0 / (1.0 + a * a - b * b)
    else:
        a, b, d = 2.0 * kappa * mu, -2.0 * kappa * epsilon, 1.0
    if dagger:
        a = -a
    h = v.size // 2
    u1, u2 = v[:h].reshape(-1, 4, 3, 2), v[h:].reshape(-1, 4, 3, 2)
    a5 = _G5 * a
    o1, o2 = np.empty_like(u1), np.empty_like(u2)
    o1[..., 0] = d * (u1[..., 0] - a5 * u1[..., 1] + b * u2[..., 0])
    o1[..., 1] = d * (u1[..., 1] + a5 * u1[..., 0] + b * u2[..., 1])
    o2[..., 0] = d * (u2[..., 0] + a5 * u2[..., 1] + b * u1[..., 0])
    o2[..., 1] = d * (u2[..., 1] - a5 * u2[..., 0] + b * u1[..., 1])
    return np.concatenate([o1.ravel(), o2.ravel()])


def _hop(oracle, gauge, v, X, parity, dagger):
    """the single-flavour hop on both flavours of a parity doublet"""
    h = v.size // 2
    return np.concatenate([oracle.wil_dslash(gauge, np.ascontiguousarray(v[:h]), list(X), parity, dagger),
                           oracle.wil_dslash(gauge, np.ascontiguousarray(v[h:]), list(X), parity, dagger)])


def ndeg_dslash(oracle, gauge, v, X, kappa, mu, epsilon, parity, matpc, dagger):
    """A^-1 D, or D^dag A^-1^dag for dagger with symmetric preconditioning"""
    if dagger and not matpc.endswith("asym"):
        return _hop(oracle, gauge, ndeg_twist(v, kappa, mu, epsilon, 1, 1), X, parity, 1)
    return ndeg_twist(_hop(oracle, gauge, v, X, parity, dagger), kappa, mu, epsilon, dagger, 1)


def ndeg_matpc(oracle, gauge, v, X, kappa, mu, epsilon, matpc, dagger):
    """1 - kappa^2 A^-1 D A^-1 D (symmetric; every factor daggered and the order reversed under dagger) or A - kappa^2 D A^-1 D (asymmetric)"""
    p0 = qc.P0[matpc]
    Ainv = lambda w: ndeg_twist(w, kappa, mu, epsilon, dagger, 1)
    D = lambda w, parity: _hop(oracle, gauge, w, X, parity, dagger)
    if matpc.endswith("asym"):
        return ndeg_twist(v, kappa, mu, epsilon, dagger, 0) + (-kappa * kappa) * D(Ainv(D(v, 1 - p0)), p0)
    if dagger:
        return v + (-kappa * kappa) * D(Ainv(D(Ainv(v), 1 - p0)), p0)
    return v + (-kappa * kappa) * Ainv(D(Ainv(D(v, 1 - p0)), p0))


def ndeg_mat(oracle, gauge, v, X, kappa, mu, epsilon, dagger):
    """A - kappa D on both parities of a full doublet"""
    h = v.size // 2
    even, odd = v[:h], v[h:]
    A = lambda w: ndeg_twist(w, kappa, mu, epsilon, dagger, 0)
    return np.concatenate([A(even) + (-kappa) * _hop(oracle, gauge, odd, X, 0, dagger), A(odd) + (-kappa) * _hop(oracle, gauge, even, X, 1, dagger)])


def host_case(oracle, name, gauge, spinor2, X, kappa, mu, epsilon):
    """the host reference of golden case `name` on the full doublet spinor2"""
    t = name.split("_")
    nd = spinor2.size // 2
    if t[1] == "dslash":
        return ndeg_dslash(oracle, gauge, spinor2[:nd], X, kappa, mu, epsilon, int(t[4][1]), t[2], int(t[3][1]))
    if t[1] == "matpc":
        p0 = qc.P0[t[2]]
        return ndeg_matpc(oracle, gauge, spinor2[p0 * nd:(p0 + 1) * nd], X, kappa, mu, epsilon, t[2], int(t[3][1]))
    if t[1] == "mat":
        return ndeg_mat(oracle, gauge, spinor2, X, kappa, mu, epsilon, int(t[2][1]))
    raise KeyError(name)


@pytest.mark.parametrize("X", LATTICES, ids=["4x4x4x4", "6x4x2x8"])
def test_goldens_load_and_continue_the_committed_spinor(X):
    z, gauge, spinor = load_golden(X)
    V = int(np.prod(X))
    assert [int(v) for v in z["meta_X"]] == list(X)
    assert (float(z["kappa"]), float(z["mu"]), float(z["epsilon"])) == (0.12, 0.3, 0.2)
    assert z["spinor2"].size == 2 * V * 24 and np.array_equal(z["spinor2"][:V * 24], spinor)
    names = case_names(z)
    assert len(names) == 26
    assert sum(n.startswith("ndeg_dslash") for n in names) == 16 and sum(n.startswith("ndeg_matpc") for n in names) == 8
    for n in names:
        assert z[n].size == (2 * V * 24 if n.startswith("ndeg_mat_") else V * 24), n


@pytest.mark.parametrize("X", LATTICES, ids=["4x4x4x4", "6x4x2x8"])
def test_composition_reproduces_the_reference_bit_for_bit(oracle, X):
    z, gauge, _ = load_golden(X)
    kappa, mu, epsilon = float(z["kappa"]), float(z["mu"]), float(z["epsilon"])
    worst = {}
    for name in case_names(z):
        got = host_case(oracle, name, gauge, z["spinor2"], X, kappa, mu, epsilon)
        worst[name] = float(np.max(np.abs(got - z[name])))
    print(worst)
    assert len(worst) == 26
    assert max(worst.values()) == 0.0, {k: v for k, v in worst.items() if v != 0.0}


@pytest.mark.parametrize("X", LATTICES, ids=["4x4x4x4", "6x4x2x8"])
def test_zero_splitting_gives_the_two_degenerate_operators(oracle, X):
    """epsilon = 0: flavour 1 is the degenerate operator of flavour +1, flavour 2 that of flavour -1.  Equality up to rounding (1e-14 of the
    largest element): the degenerate twist multiplies by 1 / (1 + a^2) where the doublet formula adds 0 * (other flavour) first."""
    z, gauge, _ = load_golden(X)
    kappa, mu = float(z["kappa"]), float(z["mu"])
    nd = z["spinor2"].size // 2
    nh = nd // 2
    v = z["spinor2"][:nd]
    for matpc in MPC:
        for dagger in (0, 1):
            for parity in (0, 1):
                got = ndeg_dslash(oracle, gauge, v, X, kappa, mu, 0.0, parity, matpc, dagger)
                for f, sign in ((0, +1), (1, -1)):
                    want = oracle.tm_dslash(gauge, v[f * nh:(f + 1) * nh].copy(), list(X), kappa, mu, sign, parity, matpc, dagger)
                    assert qc.rel_err(got[f * nh:(f + 1) * nh], want) < 1e-14, (matpc, dagger, parity, f)
