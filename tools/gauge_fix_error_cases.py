#!/usr/bin/env python3
"""Error convention of the gauge-fixing entry points: a failure prints `ERROR: ... (rank, file:line in func())` and exits with
status 1.  usage: gauge_fix_error_cases.py <case>"""
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
qa.init(0)
gp = qa.gauge_param(X, t_boundary=qa.QUDA_PERIODIC_T)
if case == "reunit_interval_zero":
    qa.gauge_fix_ovr(gp, 4, 10, 1.5, 0.0, 0, 1, gauge=unit)
elif case == "without_resident_gauge":
    qa.gauge_fix_ovr(gp, 4, 10, 1.5, 0.0, 4, 1, gauge=None)
elif case == "milc_gauge_order":
    gp.gauge_order = qa.QUDA_MILC_GAUGE_ORDER
    qa.gauge_fix_ovr(gp, 4, 10, 1.5, 0.0, 4, 1, gauge=unit)
elif case == "singular_input_link":
    bad = unit.copy()
    bad[1, 18 * 7:18 * 8] = 0.0   # one link is the zero matrix: nothing to project onto SU(3)
    qa.gauge_fix_ovr(gp, 4, 10, 1.5, 0.0, 4, 1, gauge=bad)
print("NOT REACHED: %s did not abort" % case)
