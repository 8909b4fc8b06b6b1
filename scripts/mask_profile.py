"""Time the ocean mask (csrc/ogg_mask.hip) at 1/8 and 1/16 degree on two wet sets built on the device (nothing is downloaded):

  realistic   a generated continent mask: a smooth field of a few dozen waves plus a seeded hash, wet where it is below zero: continents
              with ragged coasts, inland seas, lakes, islands and one-cell ponds (about 75 % wet)
  serpentine  the worst case: a one-cell-wide channel that winds through every other row and fills the grid (one component of half
              the cells)

    python scripts/mask_profile.py --time [--res 8 16] [--tile_rows 8 16 32 64] [--reps 20] [--json OUT] [--baseline]

Cells: the model cells of the tripolar grid (2196 x 2880 at 1/8 degree, 4392 x 5760 at 1/16), periodic and folded.  For every case and
OGG_MASK_TILE_ROWS value: HIP-event times of the label step (ogg_mask_label_dev: tile labelling, merge, flatten, component list) and
of the apply step (ogg_mask_apply_dev), median of --reps runs after one warm-up; the host's read of the counts between the two steps is
not timed.  --baseline adds the numpy definition's time (tests/ocean_mask_definition.py) on one host core at 1/8 degree.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = {8: (2196, 2880), 16: (4392, 5760)}


def wet_set(kind, ny, nx, device):
    """float64 depth (ny x nx) on the device: 100 m where wet, 0 where land"""
    import torch
    if kind == "serpentine":
        w = torch.zeros((ny, nx), dtype=torch.bool, device=device)
        w[::2] = True
        rows = torch.arange(1, ny, 2, device=device)
        cols = torch.where((torch.arange(rows.numel(), device=device) % 2) == 0, nx - 1, 0)
        w[rows, cols] = True
        return w.to(torch.float64) * 100.0
    g = torch.Generator(device=device).manual_seed(7)
    lon = (torch.arange(nx, device=device, dtype=torch.float64) + 0.5) * (360.0 / nx)
    lat = -80.0 + (torch.arange(ny, device=device, dtype=torch.float64) + 0.5) * (170.0 / ny)
    L, A = torch.deg2rad(lon)[None, :], torch.deg2rad(lat)[:, None]
    z = torch.full((ny, nx), -0.35, dtype=torch.float64, device=device)
    for k in range(36):
        a, b, c, p = (torch.rand(4, generator=g, device=device, dtype=torch.float64) * torch.tensor([1.0, 12.0, 12.0, 6.283],
                                                                                                     device=device, dtype=torch.float64))
        z += (0.5 / (1 + k // 6)) * a * torch.sin(torch.floor(b + 1) * L + p) * torch.cos(torch.floor(c + 1) * A + 0.5 * p)
    rows = torch.arange(ny, device=device, dtype=torch.int64)[:, None]
    cols = torch.arange(nx, device=device, dtype=torch.int64)[None, :]
    h = (((rows * 2654435761 + cols * 40503) ^ 0x5bd1e995) % 1001).to(torch.float64) / 1000.0 - 0.5
    z += 0.25 * h
    return torch.where(z < 0, -z * 4000.0, torch.zeros_like(z))


def run_once(p, depth, ws, root, comps, counts, kept, out, wet, st):
    import torch

    from ocean_model_grid_generator_amd import _lib as L
    e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    e[0].record()
    L.call("ogg_mask_label_dev", ctypes.byref(p), depth.data_ptr(), ws.data_ptr(), ws.numel(), root.data_ptr(), comps.data_ptr(),
           counts.data_ptr(), st)
    e[1].record()
    c = counts.cpu()   # the host's choice: the largest component
    kept.fill_(int(2**31 - 1 - (int(c[4]) & 0xFFFFFFFF)))
    e[2].record()
    L.call("ogg_mask_apply_dev", ctypes.byref(p), depth.data_ptr(), root.data_ptr(), ws.data_ptr(), ws.numel(), kept.data_ptr(),
           1 if int(c[3]) else 0, out.data_ptr(), wet.data_ptr(), counts.data_ptr(), st)
    e[3].record()
    torch.cuda.synchronize()
    return e[0].elapsed_time(e[1]), e[2].elapsed_time(e[3]), c.tolist()


def time_case(kind, res, tile_rows, reps):
    import torch

    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import ocean_mask as M
    ny, nx = SHAPES[res]
    depth = wet_set(kind, ny, nx, "cuda:0")
    p = M.params(ny, nx, True, True)
    ws = torch.empty(int(L.load().ogg_mask_workspace_bytes(ctypes.byref(p))), dtype=torch.uint8, device="cuda:0")
    root = torch.empty((ny, nx), dtype=torch.int32, device="cuda:0")
    comps = torch.empty(ny * nx, dtype=torch.int64, device="cuda:0")
    counts = torch.zeros(len(L.MASK_COUNT_FIELDS), dtype=torch.int64, device="cuda:0")
    kept = torch.zeros(1, dtype=torch.int32, device="cuda:0")
    out = torch.empty_like(depth)
    wet = torch.empty((ny, nx), dtype=torch.uint8, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    rows = []
    for rws in tile_rows:
        os.environ["OGG_MASK_TILE_ROWS"] = str(rws)
        run_once(p, depth, ws, root, comps, counts, kept, out, wet, st)   # warm-up
        t = [run_once(p, depth, ws, root, comps, counts, kept, out, wet, st) for _ in range(reps)]
        lab = sorted(a for a, _, _ in t)[reps // 2]
        app = sorted(b for _, b, _ in t)[reps // 2]
        c = dict(zip(L.MASK_COUNT_FIELDS, counts.cpu().tolist()))   # (after the last apply step: every count)
        row = {"case": kind, "res": res, "shape": [ny, nx], "tile_rows": rws, "label_ms": lab, "apply_ms": app, "total_ms": lab + app,
               "wet": c["wet_in"], "components": c["components"], "largest": c["largest"] >> 32}
        print(json.dumps(row))
        rows.append(row)
    os.environ.pop("OGG_MASK_TILE_ROWS", None)
    return rows


def baseline():
    import numpy as np
    import ocean_mask_definition as D
    d = wet_set("realistic", *SHAPES[8], "cuda:0").cpu().numpy()
    t0 = time.perf_counter()
    want = D.ocean_mask(d, periodic=True, fold=True)
    dt = time.perf_counter() - t0
    row = {"case": "realistic", "res": 8, "numpy_definition_s": dt, "components": want["n_components"], "wet": int(np.sum(d > 0))}
    print(json.dumps(row))
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--time", action="store_true", help="time the device work")
    ap.add_argument("--res", type=int, nargs="+", default=[8, 16])
    ap.add_argument("--tile_rows", type=int, nargs="+", default=[8, 16, 32, 64])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--baseline", action="store_true")
    a = ap.parse_args()
    import torch  # noqa: F401

    from ocean_model_grid_generator_amd import _lib as L
    rows = []
    if a.time:
        for res in a.res:
            for kind in ("realistic", "serpentine"):
                rows += time_case(kind, res, a.tile_rows, a.reps)
    if a.baseline:
        rows.append(baseline())
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": L.device_name(), "library": L.load().ogg_version().decode(), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
