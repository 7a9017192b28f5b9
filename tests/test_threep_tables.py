"""The spin tables of the three-point functions (qudaAmdThreepOperator, qudaAmdThreepProjector) against explicit gamma products of
the UKQCD basis, and the exported interface: no GPU needed."""
import importlib

import numpy as np

_s = [np.array([[0, 1], [1, 0]], complex), np.array([[0, -1j], [1j, 0]]), np.array([[1, 0], [0, -1]], complex)]
_Z2 = np.zeros((2, 2))
G = {k: np.block([[_Z2, 1j * _s[k - 1]], [-1j * _s[k - 1], _Z2]]) for k in (1, 2, 3)}
G[4] = np.diag([1, 1, -1, -1]).astype(complex)
G[5] = G[1] @ G[2] @ G[3] @ G[4]
ONE = np.eye(4, dtype=complex)


def operators(s):
    """O_0 .. O_15 for the flavour sign s"""
    return ([s * 1j * G[5]] + [G[k] for k in (1, 2, 3, 4)] + [s * 1j * ONE] + [G[5] @ G[k] for k in (1, 2, 3, 4)]
            + [s * G[5] @ G[a] @ G[b] for a, b in ((1, 2), (1, 3), (2, 3), (4, 1), (4, 2), (4, 3))])


def projector(pid, particle):
    """R_p Gamma R_p; pid in the order G4, G5G123, G5G1, G5G2, G5G3; particle 0 proton (p = +1), 1 neutron (p = -1)"""
    P4 = (ONE + G[4]) / 4
    g5gk = {k: P4 @ (1j * G[5] @ G[k]) for k in (1, 2, 3)}
    gam = [P4, g5gk[1] + g5gk[2] + g5gk[3], g5gk[1], g5gk[2], g5gk[3]][pid]
    R = (ONE + (1 if particle == 0 else -1) * 1j * G[5]) / np.sqrt(2)
    return R @ gam @ R


def test_symbols_are_exported():
    qa = importlib.import_module("quda-qkxtm-multigrid_amd")
    L = qa.lib()
    for name in ("qudaAmdThreepSeqSource", "qudaAmdContractThreep", "qudaAmdSetThreepOutput", "qudaAmdThreepLastTimings", "qudaAmdThreepOperator",
                 "qudaAmdThreepProjector"):
        assert hasattr(L, name), name
    for name in ("threep_seq_source", "contract_threep", "set_threep_output"):
        assert callable(getattr(qa, name)), name
    assert (qa.PROTON, qa.NEUTRON) == (0, 1)
    assert (qa.G4, qa.G5G123, qa.G5G1, qa.G5G2, qa.G5G3) == (0, 1, 2, 3, 4)


def test_operator_table_matches_the_gamma_products():
    qa = importlib.import_module("quda-qkxtm-multigrid_amd")
    for s in (+1, -1):
        want = operators(s)
        assert len(want) == 16
        for i in range(16):
            assert np.max(np.abs(qa.threep_operator(i, s) - want[i])) < 1e-15, (i, s)
    # the flavour sign enters exactly the operators 0, 5 and 10 .. 15
    flips = [i for i in range(16) if not np.array_equal(qa.threep_operator(i, +1), qa.threep_operator(i, -1))]
    assert flips == [0, 5, 10, 11, 12, 13, 14, 15]


def test_projector_table_matches_the_gamma_products():
    qa = importlib.import_module("quda-qkxtm-multigrid_amd")
    for particle in (qa.PROTON, qa.NEUTRON):
        for pid in range(5):
            got = qa.threep_projector(pid, particle)
            assert np.max(np.abs(got - projector(pid, particle))) < 1e-15, (pid, particle)
        total = sum(qa.threep_projector(pid, particle) for pid in (qa.G5G1, qa.G5G2, qa.G5G3))
        assert np.max(np.abs(qa.threep_projector(qa.G5G123, particle) - total)) < 1e-15
    assert not np.allclose(qa.threep_projector(qa.G4, qa.PROTON), qa.threep_projector(qa.G4, qa.NEUTRON))
