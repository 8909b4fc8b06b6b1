"""Cost of Supergrid.topography against a REGIONAL raster: the r2_nosc grid and the float64 regional raster of tests/test_gpu_topog.py
(31 M samples, most of them outside the raster, where the regional index pays its fmod), timed as a host clock around the call ending in
a device synchronise, 3 warm-up and 20 timed calls; one JSON line.  OGG_LIB_PATH names another build of the library (the parent's, for
parent / change / parent in one session); under rocprofv3 --kernel-trace --stats the kernel's own time is topog_band_kernel's.

    [OGG_LIB_PATH=parent/libogg_hip.so] python scripts/topog_regional_time.py LABEL
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

import ocean_model_grid_generator_amd.supergrid as sg
from ocean_model_grid_generator_amd import topography as T
from test_gpu_topog import CONFIGS, raster

plan = sg.SupergridPlan(**CONFIGS["r2_nosc"])
g = sg.Supergrid(plan, device="cuda:0")
g.run_pass()
data, box, fill = raster("float64_regional")
dev = T.DeviceSource(T.Source(data, *box, fill=fill), "cuda:0")
cut = g.south_cut()
times = []
for k in range(23):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = g.topography(cut, dev)
    torch.cuda.synchronize()
    times.append(time.perf_counter() - t0)
t = np.array(times[3:]) * 1e3
print(json.dumps({"label": sys.argv[1] if len(sys.argv) > 1 else "", "lib": os.environ.get("OGG_LIB_PATH", "tree"),
                  "n_samples": res["summary"]["n_samples"], "n_valid": res["summary"]["n_valid_samples"],
                  "median_ms": round(float(np.median(t)), 4), "min_ms": round(float(t.min()), 4), "max_ms": round(float(t.max()), 4),
                  "runs": len(t)}))
