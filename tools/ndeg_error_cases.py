#!/usr/bin/env python3
"""What the library refuses for the non-degenerate twisted-mass doublet: each case ends the process with `ERROR: ...` and exit status 1
(the convention of tools/error_cases.py).  usage: ndeg_error_cases.py <case>"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
qa = importlib.import_module("quda-qkxtm-multigrid_amd")
case = sys.argv[1]
X = [4, 4, 4, 4]
V = int(np.prod(X))
DBL = qa.QUDA_TWIST_NONDEG_DOUBLET
qa.init(0)
unit = np.zeros((4, V, 9, 2))
unit[:, :, [0, 4, 8], 0] = 1
qa.load_gauge(unit.reshape(4, -1), qa.gauge_param(X, t_boundary=qa.QUDA_PERIODIC_T))
if case == "twisted_clover":
    ip = qa.invert_param(qa.QUDA_TWISTED_CLOVER_DSLASH, 0.12, 0.3, +1, epsilon=0.2)
    ip.clover_coeff = 0.1
    qa.load_clover(None, None, ip)
    ip.twist_flavor = DBL
    qa.dslash(np.ones(V * 24), ip, 0)
elif case == "multigrid":
    ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, 0.12, 0.3, DBL, solution_type=qa.QUDA_MAT_SOLUTION, epsilon=0.2)
    ip.solve_type, ip.inv_type, ip.gcrNkrylov, ip.tol, ip.maxiter = qa.QUDA_DIRECT_SOLVE, qa.QUDA_GCR_INVERTER, 10, 1e-6, 100
    qa.Multigrid(qa.multigrid_param(ip, n_level=2, geo_block=(2, 2, 2, 2), n_vec=4, setup_maxiter=5, setup_tol=1e-1))
elif case == "multi_src":
    ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, 0.12, 0.3, DBL, solution_type=qa.QUDA_MAT_SOLUTION, epsilon=0.2)
    ip.solve_type, ip.inv_type, ip.gcrNkrylov, ip.tol, ip.maxiter = qa.QUDA_DIRECT_PC_SOLVE, qa.QUDA_GCR_INVERTER, 10, 1e-6, 100
    qa.invert_multi_src([np.ones(2 * V * 24), np.ones(2 * V * 24)], ip)
elif case == "no_inverse":   # 1 + a^2 - b^2 <= 0 with a = 2 kappa mu, b = 2 kappa epsilon
    ip = qa.invert_param(qa.QUDA_TWISTED_MASS_DSLASH, 0.12, 0.3, DBL, epsilon=5.0)
    qa.dslash(np.ones(V * 24), ip, 0)
elif case == "change_twist":
    f = qa.Spinor(8, flavor=+1)
    qa.lib().qudaAmdSpinorSetTwist(f.h, DBL)
print("NOT REACHED: %s did not abort" % case)
