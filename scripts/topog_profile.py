"""Time topography by refined sampling (csrc/ogg_topog.hip) on generated grids against a synthetic int16 raster of GEBCO size built
on the device (a smooth analytic field plus a seeded hash: nothing is downloaded).

    python scripts/topog_profile.py [--res 8] [--arcsec 30 15] [--dp 0 0.2] [--reps 3] [--json OUT] [--baseline] [--plane] [--int32]

For every (raster, grid) pair: HIP-event times of the sampling of the whole stitched grid (Supergrid.topography_records: every
band's ogg_topog_band_dev; the halo rows are fetched once before the timed runs and are not timed), samples, samples/s.  --baseline adds the numpy definition's samples/s on one host
core (tests/topog_definition.py, on a small grid against the same kind of raster).  One warm-up run precedes the timed ones.
--plane times the plane-fit kernel (ogg_topog_plane_band_dev) as well, in the same process: after a warm-up of each, every repetition
runs the base sampling and then the plane sampling, so that both see the same box at the same time; it reports both lists of times,
the ratio of the best and of the median times, and checks that the base half of the plane records is the base records.
--int32 widens the raster to int32 quanta on the device (what a float source becomes once quantised), so that the int32 instantiations
of both kernels are the ones timed.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synthetic_raster(arcsec, device):
    """(int16 device tensor Ny x Nx, box): global raster of `arcsec` seconds, cell edges from (-180, -90)."""
    import torch
    n_per_deg = 3600 // arcsec
    Nx, Ny = 360 * n_per_deg, 180 * n_per_deg
    out = torch.empty((Ny, Nx), dtype=torch.int16, device=device)
    lon = (torch.arange(Nx, device=device, dtype=torch.float64) + 0.5) / n_per_deg - 180.0
    slon = torch.sin(torch.deg2rad(3.0 * lon))
    cols = torch.arange(Nx, device=device, dtype=torch.int64)
    step = 2048
    for j0 in range(0, Ny, step):
        j1 = min(Ny, j0 + step)
        lat = (torch.arange(j0, j1, device=device, dtype=torch.float64) + 0.5) / n_per_deg - 90.0
        z = 4000.0 * slon[None, :] * torch.cos(torch.deg2rad(2.0 * lat))[:, None] - 1500.0
        rows = torch.arange(j0, j1, device=device, dtype=torch.int64)
        h = ((rows[:, None] * 2654435761 + cols[None, :] * 40503) ^ 0x5bd1e995) % 301 - 150
        out[j0:j1] = (z + h.to(torch.float64)).to(torch.int16)
    return out, (-180.0, 1.0 / n_per_deg, -90.0, 1.0 / n_per_deg)


class _DeviceRaster(object):
    """A topography.DeviceSource over a raster that already lives on the device."""

    def __init__(self, tensor, box, int32=False):
        import numpy as np
        import torch

        from ocean_model_grid_generator_amd import _lib as L
        from ocean_model_grid_generator_amd import topography as T
        if int32:
            tensor = tensor.to(torch.int32)
        self.tensor, self.sea_level = tensor, 0.0
        self.source = T.Source(np.zeros((1, 1), dtype=np.int16), *box)
        Ny, Nx = tensor.shape
        self.desc = L.TopogSource(data=tensor.data_ptr(), dtype=L.TOPOG_INT32 if int32 else L.TOPOG_INT16, n_fill=0, Nx=Nx, Ny=Ny, lon0=box[0], dlon=box[1],
                                  lat0=box[2], dlat=box[3], quantum=1.0, wet_below=0.0)


def time_grid(res, r_dp, src, reps, plane=False):
    import torch

    from ocean_model_grid_generator_amd import supergrid as SG
    plan = SG.SupergridPlan(inverse_resolution=res, r_dp=r_dp, ensure_nj_even=True)
    g = SG.Supergrid(plan, device="cuda:0")
    g.run_pass()
    cut = g.south_cut()
    halo = g.quality_halo(cut)
    recs = g.topography_records(cut, src, halo=halo)   # warm-up
    samples = sum(int((t[..., 0] + t[..., 1]).sum()) for _, _, t in recs)
    r_max = max(int((t[..., 6] & 0xFFFFFFFF).max()) for _, _, t in recs)   # the low half of word 6 is R
    del recs
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        recs = g.topography_records(cut, src, halo=halo)
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1))
        del recs
    best = min(times)
    out = {"res": res, "r_dp": r_dp, "nyp": g.stitched_rows(cut), "nxp": plan.Ni + 1, "samples": samples, "R_max": r_max,
           "ms": times, "ms_best": best, "samples_per_s": samples / (best * 1e-3)}
    if plane:
        base = g.topography_records(cut, src, halo=halo)
        recs = g.topography_records(cut, src, halo=halo, plane=True)   # warm-up of the plane kernel
        out["base_half_equal"] = all(bool((b == p[..., :7]).all()) for (_, _, b), (_, _, p) in zip(base, recs))
        out["n_far"] = sum(int(t[..., 14].sum()) for _, _, t in recs)
        del base, recs
        tb, tp = [], []
        for _ in range(reps):
            for flag, times in ((False, tb), (True, tp)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                recs = g.topography_records(cut, src, halo=halo, plane=flag)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
                del recs
        med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
        out.update(ms_base_alternating=tb, ms_plane=tp, ms_plane_best=min(tp), ratio_best=min(tp) / min(tb), ratio_median=med(tp) / med(tb))
    return out


def baseline(arcsec_like=30):
    """Samples/s of the numpy definition on one core: a -r 1 lat-lon strip against a small raster of the same R."""
    import numpy as np
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import topog_definition as td
    d = 0.25
    x, y = np.meshgrid(-180.0 + 0.5 * np.arange(721), -60.0 + 0.5 * np.arange(41))
    raw = (np.arange(720 * 1440) % 3001 - 1500).astype(np.int16).reshape(720, 1440)
    t0 = time.perf_counter()
    r = td.supergrid_records(x, y, td.quantise(raw)[0], -180.0, d, -90.0, d, refine=30)
    dt = time.perf_counter() - t0
    n = int((r["n"] + r["n_missing"]).sum())
    return {"samples": n, "s": dt, "samples_per_s": n / dt, "R": 30}


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("--res", type=float, nargs="+", default=[8.0])
    p.add_argument("--arcsec", type=int, nargs="+", default=[30, 15])
    p.add_argument("--dp", type=float, nargs="+", default=[0.0, 0.2])
    p.add_argument("--reps", type=int, default=3)
    p.add_argument("--json", default=None)
    p.add_argument("--baseline", action="store_true")
    p.add_argument("--plane", action="store_true", help="also time the plane-fit kernel, alternating with the base kernel")
    p.add_argument("--int32", action="store_true", help="sample the raster as int32 quanta (the kernels of a quantised float source)")
    a = p.parse_args(argv)
    import torch
    out = []
    for arcsec in a.arcsec:
        t, box = synthetic_raster(arcsec, "cuda:0")
        torch.cuda.synchronize()
        src = _DeviceRaster(t, box, a.int32)
        for res in a.res:
            for dp in a.dp:
                r = time_grid(res, dp, src, a.reps, a.plane)
                r["arcsec"] = arcsec
                r["dtype"] = "int32" if a.int32 else "int16"
                r["raster"] = list(t.shape)
                print(json.dumps(r))
                out.append(r)
        del src, t
        torch.cuda.empty_cache()
    if a.baseline:
        b = baseline()
        print(json.dumps({"numpy_baseline": b}))
        out.append({"numpy_baseline": b})
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
