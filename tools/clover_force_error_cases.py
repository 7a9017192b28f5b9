#!/usr/bin/env python3
"""Refusals of the twisted-clover force entry points: a failure prints `ERROR: ... (rank, file:line in func())` and exits with status 1,
before any device work of the force.  usage: clover_force_error_cases.py <case>"""
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
unit = np.zeros((4, V, 9, 2))
unit[:, :, [0, 4, 8], 0] = 1
unit = unit.reshape(4, -1)
kappa, mu = 0.13, 0.2
x = [np.random.default_rng(1).standard_normal(V * 12)]
mom = np.zeros((V, 4, 10))
qa.init(0)
if case.startswith("partitioned"):
    qa.lib().qudaAmdSetPartitionMask(0b1010)
gp = qa.gauge_param(X, t_boundary=qa.QUDA_PERIODIC_T)
qa.load_gauge(unit, gp)
flavor = qa.QUDA_TWIST_NONDEG_DOUBLET if case == "doublet" else qa.QUDA_TWIST_PLUS
ip = qa.invert_param(qa.QUDA_TWISTED_CLOVER_DSLASH, kappa, mu, flavor, "ee", 0, solution_type=qa.QUDA_MATPCDAG_MATPC_SOLUTION)
ip.solve_type = qa.QUDA_NORMOP_PC_SOLVE
ip.clover_coeff = kappa * 1.57551
if case == "partitioned_derivative":
    qa.clover_derivative_force(gp, np.zeros((V, 6, 3, 3, 2)), 1.0, mom=mom)
elif case == "partitioned_tm_force":
    qa.load_clover(None, None, ip)
    qa.tm_force(gp, ip, x, [1.0], 0.1, mom=mom)
elif case == "partitioned_logdet":
    qa.load_clover(None, None, ip)
    qa.clover_logdet_force(gp, ip, 0.1, 0.0, -1.0, mom=mom)
elif case == "clover_from_the_host":
    packed = np.zeros((V, 2, 36))
    packed[:, :, :6] = 1.0
    qa.load_clover(packed.reshape(-1), None, ip)
    qa.tm_force(gp, ip, x, [1.0], 0.1, mom=mom)
elif case == "another_clover_coeff":
    qa.load_clover(None, None, ip)
    ip.clover_coeff = 1.1 * ip.clover_coeff
    qa.clover_logdet_force(gp, ip, 0.1, 0.0, -1.0, mom=mom)
elif case == "another_mu":
    qa.load_clover(None, None, ip)
    ip.mu = 2.0 * mu
    qa.tm_force(gp, ip, x, [1.0], 0.1, mom=mom)
elif case == "clover_not_fp64":
    ip.clover_cuda_prec = qa.QUDA_SINGLE_PRECISION
    qa.load_clover(None, None, ip)
    qa.clover_sigma_trace(ip, 1.0, 1.0, V)
elif case == "no_clover_term":
    qa.tm_force(gp, ip, x, [1.0], 0.1, mom=mom)
elif case == "doublet":
    qa.tm_force(gp, ip, [np.zeros(V * 24)], [1.0], 0.1, mom=mom)
print("NOT REACHED: %s did not abort" % case)
