"""Time the sill depths (csrc/ogg_sill.hip) on one GPU (nothing is downloaded), on the cases of scripts/coast_distance_profile.py:

  om4   the generated 1/4-degree (OM4 flags) tripolar grid with the synthetic continents of the tests
  r8    a regular 1/8-degree lat-lon supergrid of 2196 x 2880 model cells (periodic) with the generated-continent wet set of
        scripts/mask_profile.py

    python scripts/sill_profile.py [--cases om4 r8] [--reps 10] [--json OUT]

in ``cells`` mode with 0.01 m quanta, under a synthetic bottom (DEPTH below: a smooth ocean floor 200 .. 5700 m deep with ridges, so
the plane has many sill levels and regions).  For every case: HIP-event times of a whole ogg_sill_depth_dev call alternating in one
process with ogg_mask_label_dev on the same wet set; the rounds; the time per round (the whole call over the rounds: the set-up, the
last labelling and the gates are counted in); and the ratio of the time per round to one mask labelling.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from basin_codes_profile import Label   # noqa: E402
from coast_distance_profile import case_grid, ev, stats   # noqa: E402

QUANTUM = 0.01


def depth_of(x, y, wet):
    """DEPTH: metres, positive down, 0 on land"""
    import torch
    lon, lat = torch.deg2rad(x[1::2, 1::2]), torch.deg2rad(y[1::2, 1::2])
    d = 2950.0 + 1500.0 * torch.sin(3.0 * lon) * torch.cos(2.0 * lat) + 900.0 * torch.sin(11.0 * lon + 2.0 * lat) * torch.cos(7.0 * lat) \
        + 350.0 * torch.sin(37.0 * lon) * torch.sin(29.0 * lat)
    return torch.where(wet != 0, d.clamp(min=200.0), torch.zeros_like(d)).contiguous()


class Sill(object):
    """the buffers of one case, and the call"""

    def __init__(self, x, y, wet, periodic, fold):
        import torch
        from ocean_model_grid_generator_amd import _lib as L
        from ocean_model_grid_generator_amd import sill_depth as SD
        self.L, dev = L, x.device
        self.wet = wet
        self.x, self.y = x, y
        self.ny, self.nx = wet.shape
        q = SD.quantise(depth_of(x, y, wet), QUANTUM)
        wu, wv = SD.cell_face_weights(q, periodic, fold)
        self.bits = SD.bits_for(max(int(wu.max()), int(wv.max())))
        self.wu, self.wv = wu.to(torch.int32).contiguous(), wv.to(torch.int32).contiguous()
        self.seeds = torch.tensor([SD.default_seed(q.cpu().numpy())], dtype=torch.int64, device=dev)
        self.p = SD.params(self.ny, self.nx, periodic, fold, self.bits, 1)
        self.wsb = int(L.load().ogg_sill_workspace_bytes(self.ny, self.nx))
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=dev)
        self.b = torch.empty((self.ny, self.nx), dtype=torch.int32, device=dev)
        self.region = torch.empty((self.ny, self.nx), dtype=torch.int32, device=dev)
        self.gu = torch.empty((self.ny, self.nx + 1), dtype=torch.uint8, device=dev)
        self.gv = torch.empty((self.ny + 1, self.nx), dtype=torch.uint8, device=dev)
        self.counts = torch.empty(len(L.SILL_COUNT_FIELDS), dtype=torch.int64, device=dev)
        self.st = torch.cuda.current_stream().cuda_stream

    def timed(self):
        import torch
        a, b = ev(), ev()
        a.record()
        self.L.call("ogg_sill_depth_dev", *self.p, self.wu.data_ptr(), self.wv.data_ptr(), self.seeds.data_ptr(),
                    self.ws.data_ptr(), self.wsb, self.b.data_ptr(), self.region.data_ptr(), self.gu.data_ptr(), self.gv.data_ptr(),
                    self.counts.data_ptr(), self.st)
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["om4", "r8"], choices=["r2", "om4", "r8"])
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    import torch

    from ocean_model_grid_generator_amd import _lib as L
    rows = []
    for name in a.cases:
        x, y, wet, periodic, fold = case_grid(name, "cuda:0")
        s = Sill(x, y, wet, periodic, fold)
        lab = Label(s, periodic, fold)
        t_sill, t_lab, first = [], [], None
        for rep in range(a.reps + 1):   # alternating, the first pair a warm-up
            t1, t2 = s.timed(), lab.timed()
            if rep:
                t_sill.append(t1)
                t_lab.append(t2)
            out = (s.b.clone(), s.region.clone(), s.gu.clone(), s.gv.clone(), s.counts.clone())
            first = first or out
            assert all(torch.equal(p, q) for p, q in zip(first, out)), "two runs differ"
        counts = L.counts_dict(L.SILL_COUNT_FIELDS, s.counts)
        m = lambda v: stats(v)["median"]   # noqa: E731
        per_round = m(t_sill) / counts["rounds"]
        row = dict(case=name, shape=[s.ny, s.nx], periodic=periodic, fold=fold, reps=a.reps, quantum=QUANTUM, bits=s.bits,
                   wet_cells=int((wet != 0).sum()), sill_ms=stats(t_sill), label_ms=stats(t_lab), per_round_ms=per_round,
                   per_round_over_label=per_round / m(t_lab), levels=int(torch.unique(s.b).numel()), **counts)
        print(json.dumps(row), flush=True)
        rows.append(row)
        del s, lab
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": L.device_name(), "library": L.load().ogg_version().decode(), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
