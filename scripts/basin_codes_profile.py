"""Time the basin codes (csrc/ogg_basin.hip) on one GPU (nothing is downloaded), on the cases of scripts/coast_distance_profile.py:

  om4   the generated 1/4-degree (OM4 flags) tripolar grid with the synthetic continents of the tests
  r8    a regular 1/8-degree lat-lon supergrid of 2196 x 2880 model cells (periodic) with the generated-continent wet set of
        scripts/mask_profile.py

    python scripts/basin_codes_profile.py [--cases om4 r8] [--reps 20] [--json OUT]

under a hand-written table of 20 rules (RULES below: a southern ring, six tropical and six northern sectors and an Arctic cap that
share one pass, then overlapping catch-all bands).  For every case: the passes planned against the rules; HIP-event times of a whole
call, batched and with OGG_BASIN_BATCH=0, alternating in one process (and whether the two gave the same bytes); the time of a call
with ONE rule whose box is the whole sphere (the set-up, unit vectors and seed search, and one pass over the whole wet plane)
alternating with ogg_mask_label_dev on the same wet plane; and the mean cost of a further pass, (unbatched - batched) / (passes
saved).
"""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from coast_distance_profile import case_grid, ev, stats   # noqa: E402

FULL = (-180.0, 180.0, -90.0, 90.0)
RULES = [(1, -150.0, -60.0, -180.0, 180.0, -90.0, -35.0, "southern")] + \
    [(2 + k, 60.0 * k + 29.0, -10.0, 60.0 * k, 60.0 * k + 58.0, -35.0, 30.0, "tropics_%d" % k) for k in range(6)] + \
    [(8 + k, 60.0 * k + 30.0, 45.0, 60.0 * k + 10.0, 60.0 * k + 50.0, 30.5, 65.0, "north_%d" % k) for k in range(6)] + \
    [(14, 0.0, 75.0, -180.0, 180.0, 65.5, 90.0, "arctic")] + \
    [(15 + k, -170.0 + 70.0 * k, -20.0 + 10.0 * k, -180.0, 180.0, -60.0 + 20.0 * k, min(90.0, 20.0 + 20.0 * k), "band_%d" % k) for k in range(5)] + \
    [(20, 10.0, 10.0) + FULL + ("rest",)]


class Basin(object):
    """the buffers of one case under a rule table, and the call"""

    def __init__(self, x, y, wet, periodic, fold, rules):
        import torch
        from ocean_model_grid_generator_amd import _lib as L
        from ocean_model_grid_generator_amd import basin_codes as BC
        self.L, dev = L, x.device
        self.x, self.y, self.wet = x, y, wet
        self.ny, self.nx = wet.shape
        self.rules = BC.rules_of(rules)
        self.p = BC.params(self.ny, self.nx, self.rules, periodic, fold)
        self.wsb = int(L.load().ogg_basin_workspace_bytes(ctypes.byref(self.p)))
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=dev)
        self.rt = torch.from_numpy(self.rules.table.view("uint8")).to(dev)
        self.code = torch.empty((self.ny, self.nx), dtype=torch.uint8, device=dev)
        self.rule = torch.empty((self.ny, self.nx), dtype=torch.int16, device=dev)
        self.rec = torch.empty(len(self.rules) * L.BASIN_RECORD.itemsize, dtype=torch.uint8, device=dev)
        self.counts = torch.zeros(len(L.BASIN_COUNT_FIELDS), dtype=torch.int64, device=dev)
        self.st = torch.cuda.current_stream().cuda_stream

    def call(self):
        self.L.call("ogg_basin_codes_dev", ctypes.byref(self.p), self.rules.table.ctypes.data, self.rt.data_ptr(), self.x.data_ptr(),
                    self.y.data_ptr(), 2 * self.nx + 1, self.wet.data_ptr(), self.ws.data_ptr(), self.wsb, self.code.data_ptr(),
                    self.rule.data_ptr(), self.rec.data_ptr(), self.counts.data_ptr(), self.st)

    def timed(self):
        import torch
        a, b = ev(), ev()
        a.record()
        self.call()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)

    def outputs(self):
        return self.code.clone(), self.rule.clone(), self.rec.clone()


class Label(object):
    """ogg_mask_label_dev on the wet plane of a Basin"""

    def __init__(self, b, periodic, fold):
        import torch
        from ocean_model_grid_generator_amd import ocean_mask as M
        self.L, dev = b.L, b.x.device
        self.p = M.params(b.ny, b.nx, periodic, fold)
        self.depth = b.wet.to(torch.float64).contiguous()
        self.wsb = int(self.L.load().ogg_mask_workspace_bytes(ctypes.byref(self.p)))
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=dev)
        self.root = torch.empty((b.ny, b.nx), dtype=torch.int32, device=dev)
        self.comps = torch.empty(b.ny * b.nx, dtype=torch.int64, device=dev)
        self.counts = torch.zeros(len(self.L.MASK_COUNT_FIELDS), dtype=torch.int64, device=dev)
        self.st = b.st

    def timed(self):
        import torch
        a, b = ev(), ev()
        a.record()
        self.L.call("ogg_mask_label_dev", ctypes.byref(self.p), self.depth.data_ptr(), self.ws.data_ptr(), self.wsb, self.root.data_ptr(),
                    self.comps.data_ptr(), self.counts.data_ptr(), self.st)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["om4", "r8"], choices=["r2", "om4", "r8"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch

    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import basin_codes as BC
    rows = []
    for name in a.cases:
        x, y, wet, periodic, fold = case_grid(name, "cuda:0")
        b = Basin(x, y, wet, periodic, fold, RULES)
        batched, single, outs = [], [], {}
        for rep in range(a.reps + 1):   # alternating, the first pair a warm-up
            for env, dst in (("1", batched), ("0", single)):
                os.environ["OGG_BASIN_BATCH"] = env
                t = b.timed()
                if rep:
                    dst.append(t)
                outs[env] = b.outputs() + (b.counts.cpu().tolist(),)
        del os.environ["OGG_BASIN_BATCH"]
        same = all(torch.equal(p, q) for p, q in zip(outs["1"][:3], outs["0"][:3]))
        counts = dict(zip(L.BASIN_COUNT_FIELDS, outs["1"][3]))
        rec = outs["1"][2].cpu().numpy().view(L.BASIN_RECORD)
        one = Basin(x, y, wet, periodic, fold, [(1, -150.0, -60.0) + FULL])
        lab = Label(b, periodic, fold)
        t_one, t_lab = [], []
        for rep in range(a.reps + 1):
            t1, t2 = one.timed(), lab.timed()
            if rep:
                t_one.append(t1)
                t_lab.append(t2)
        saved = len(RULES) - counts["passes"]
        m = lambda v: stats(v)["median"]   # noqa: E731
        row = dict(case=name, shape=[b.ny, b.nx], periodic=periodic, fold=fold, reps=a.reps, rules=len(RULES), plan=BC.plan(RULES),
                   n_passes=counts["passes"], passes_unbatched=outs["0"][3][3], batched_ms=stats(batched), unbatched_ms=stats(single),
                   same_bytes=same, one_rule_call_ms=stats(t_one), label_ms=stats(t_lab), one_rule_call_over_label=m(t_one) / m(t_lab),
                   further_pass_ms=(m(single) - m(batched)) / saved if saved else None,
                   further_pass_over_label=(m(single) - m(batched)) / saved / m(t_lab) if saved else None,
                   statuses=rec["status"].tolist(), cells=rec["cells"].tolist(), one_rule_cells=int(one.counts.cpu().tolist()[1]), **counts)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del b, one, lab
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": L.device_name(), "library": L.load().ogg_version().decode(), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
