"""The momentum list of the two-point functions (reference createMomenta, lib/qudaQKXTM_Kepler_kernels.cu:96-114): no GPU needed."""
import importlib

import numpy as np


def test_twop_momenta_counts_and_order():
    qa = importlib.import_module("quda-qkxtm-multigrid_amd")
    assert [len(qa.twop_momenta(q)) for q in range(5)] == [1, 7, 19, 27, 33]
    m = qa.twop_momenta(4)
    assert m[0].tolist() == [0, 0, 0]
    assert m[1:7].tolist() == [[1, 0, 0], [0, 1, 0], [0, 0, 1], [0, 0, -1], [0, -1, 0], [-1, 0, 0]]
    # shells in increasing |n|^2, each exactly the vectors of that norm, in descending lexicographic (nx, ny, nz) order
    n2 = (m ** 2).sum(axis=1)
    assert np.all(np.diff(n2) >= 0)
    for q in range(5):
        shell = [tuple(v) for v in m[n2 == q]]
        assert shell == sorted(shell, reverse=True) and len(set(shell)) == len(shell)
