#!/usr/bin/env python3
"""Error convention of the stout-smearing / topological-charge entry points: a failure prints `ERROR: ... (rank, file:line in func())`
and exits with status 1.  usage: gauge_obs_error_cases.py <case>"""
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
qa.init(0)
if case == "stout_without_gauge":
    qa.perform_stout(1, 0.1)
elif case == "charge_without_gauge":
    qa.q_charge()
elif case == "charge_of_missing_smeared_field":
    unit = np.zeros((4, V, 9, 2))
    unit[:, :, [0, 4, 8], 0] = 1
    qa.load_gauge(unit.reshape(4, -1), qa.gauge_param(X))
    assert qa.q_charge(which=0) == 0.0 and qa.q_charge() == 0.0   # the resident links are there
    qa.q_charge(which=1)
print("NOT REACHED: %s did not abort" % case)
