#!/usr/bin/env python3
"""Error convention of the gauge molecular-dynamics entry points: a failure prints `ERROR: ... (rank, file:line in func())` and exits
with status 1.  usage: gauge_md_error_cases.py <case>"""
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
staple = [[[(mu + 1) % 4, 7 - mu, 7 - (mu + 1) % 4]] for mu in range(4)]
qa.init(0)
gp = qa.gauge_param(X, t_boundary=qa.QUDA_PERIODIC_T)
if case == "force_without_resident_gauge":
    qa.gauge_force(gp, staple, [1.0], 0.1, gauge=None, mom=np.zeros((V, 4, 10)))
elif case == "action_without_resident_momentum":
    qa.load_gauge(unit, gp)
    qa.mom_action(gp, None)
elif case == "milc_gauge_order":
    gp.gauge_order = qa.QUDA_MILC_GAUGE_ORDER
    qa.update_gauge(gp, 0.1, gauge=unit, mom=np.zeros((V, 4, 10)))
elif case == "path_longer_than_the_cap":
    long_path = [[[(mu + 1) % 4] * 4 + [7 - mu] + [7 - (mu + 1) % 4] * 4] for mu in range(4)]   # 9 links
    qa.gauge_force(gp, long_path, [1.0], 0.1, gauge=unit, mom=np.zeros((V, 4, 10)))
elif case == "projection_to_zero_tolerance":
    noise = np.random.default_rng(1).standard_normal(unit.shape)
    qa.project_su3(gp, 0.0, gauge=unit + 1e-3 * noise)
print("NOT REACHED: %s did not abort" % case)
