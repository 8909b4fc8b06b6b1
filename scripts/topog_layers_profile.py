"""Time layered topography (csrc/ogg_topog.hip, topog_layers_kernel) on a generated grid against synthetic rasters built on the device
(nothing is downloaded): a global int16 raster of 15 arc seconds, and a 500 m south-polar-stereographic int16 raster of BedMachine
Antarctica's extent (13333 x 13333 elements around the pole, lat_ts = -71, lon0 = 0, WGS84).

    python scripts/topog_layers_profile.py --time [--res 8] [--arcsec 15] [--polar_m 500] [--reps 5] [--json OUT]
    python scripts/topog_layers_profile.py --once c [--res 8] ...      (one run of one variant and nothing else: for a counter run)

--time: after a warm-up of each, every repetition runs, one after the other in one process, so that all see the same box at the same
time,
    (a) the single-source kernel (ogg_topog_band_dev) on the global raster,
    (b) the layers kernel (ogg_topog_layers_band_dev) on that raster as a list of one,
    (c) the layers kernel on the polar raster over the global one,
each over the whole stitched grid (Supergrid.topography_records: every band's launch; the halo rows are fetched once, untimed), with
HIP events.  It reports the times, the samples and the samples each layer gave, checks that (b)'s records are (a)'s, and derives
ns per sample of (a) and (b), the time (c) spends beyond (b)'s rate on its lat-lon samples, and from it the cost of a projected sample.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

POLAR_EXTENT_M = 3333250.0      # BedMachine Antarctica: x, y from -3333000 to 3333000 in 500 m steps, as cell centres


def synthetic_polar(d, device):
    """(int16 device tensor N x N, box X0 dX Y0 dY): a smooth field of the plane plus a seeded hash, -1 (the fill) outside 2900 km"""
    import torch
    N = int(round(2.0 * POLAR_EXTENT_M / d))
    out = torch.empty((N, N), dtype=torch.int16, device=device)
    X = -POLAR_EXTENT_M + d * (torch.arange(N, device=device, dtype=torch.float64) + 0.5)
    cols = torch.arange(N, device=device, dtype=torch.int64)
    step = 1024
    for j0 in range(0, N, step):
        j1 = min(N, j0 + step)
        Y = -POLAR_EXTENT_M + d * (torch.arange(j0, j1, device=device, dtype=torch.float64) + 0.5)
        z = 1500.0 * torch.sin(X[None, :] / 4.0e5) * torch.cos(Y[:, None] / 3.0e5) + 200.0
        rows = torch.arange(j0, j1, device=device, dtype=torch.int64)
        h = ((rows[:, None] * 2654435761 + cols[None, :] * 40503) ^ 0x5bd1e995) % 101
        v = (z + h.to(torch.float64)).to(torch.int16)
        v[torch.hypot(X[None, :], Y[:, None]) > 2.9e6] = -1
        out[j0:j1] = v
    return out, (-POLAR_EXTENT_M, d, -POLAR_EXTENT_M, d)


class _DeviceLayers(object):
    """What Supergrid.topography_records samples (a topography.DeviceSourceList) over rasters that already live on the device:
    [(tensor, box, projection or None, lat_gate, fill)]"""

    def __init__(self, parts):
        import numpy as np

        from ocean_model_grid_generator_amd import _lib as L
        from ocean_model_grid_generator_amd import topography as T
        self.tensors, self.sea_level = [p[0] for p in parts], 0.0
        self.desc = (L.TopogLayer * len(parts))()
        stub = np.zeros((1, 1), dtype=np.int16)
        srcs = []
        for k, (t, box, proj, gate, fill) in enumerate(parts):
            Ny, Nx = t.shape
            self.desc[k].src = L.TopogSource(data=t.data_ptr(), dtype=L.TOPOG_INT16, n_fill=len(fill), Nx=Nx, Ny=Ny, lon0=box[0], dlon=box[1],
                                             lat0=box[2], dlat=box[3], quantum=1.0, wet_below=0.0)
            for i, f in enumerate(fill):
                self.desc[k].src.fill[i] = f
            self.desc[k].kind, self.desc[k].q_mul = (L.TOPOG_LATLON if proj is None else L.TOPOG_POLAR_STEREO), 1
            if proj is not None:
                self.desc[k].proj = proj.descriptor(gate)
            srcs.append(T.Source(stub, *box, projection=proj, lat_gate=gate, name="layer%d" % k))
        self.source = T.SourceList(srcs)


def run(g, cut, halo, src):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    recs = g.topography_records(cut, src, halo=halo)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), recs


def counts(recs):
    """samples, valid samples and (merge records) the samples per layer, over the pieces"""
    n = sum(int(t[..., 0].sum()) for _, _, t in recs)
    nm = sum(int(t[..., 1].sum()) for _, _, t in recs)
    out = {"samples": n + nm, "valid": n}
    if recs and recs[0][2].shape[2] == 11:
        out["n_from"] = [sum(int(t[..., 7 + k].sum()) for _, _, t in recs) for k in range(4)]
    return out


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--time", action="store_true")
    p.add_argument("--once", choices=("a", "b", "c"), default=None)
    p.add_argument("--res", type=float, default=8.0)
    p.add_argument("--arcsec", type=int, default=15)
    p.add_argument("--polar_m", type=float, default=500.0)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--json", default=None)
    a = p.parse_args(argv)
    if not a.time and not a.once:
        p.error("--time or --once")
    import torch

    from ocean_model_grid_generator_amd import supergrid as SG
    from ocean_model_grid_generator_amd import topography as T
    from topog_profile import _DeviceRaster, synthetic_raster
    want = ("a", "b", "c") if a.time else (a.once,)
    glob, gbox = synthetic_raster(a.arcsec, "cuda:0")
    variants = {}
    if "a" in want:
        variants["a"] = _DeviceRaster(glob, gbox)
    if "b" in want:
        variants["b"] = _DeviceLayers([(glob, gbox, None, None, ())])
    if "c" in want:
        polar, pbox = synthetic_polar(a.polar_m, "cuda:0")
        proj = T.PolarStereo("S", -71.0, 0.0)
        gate = float(proj.pole_latitude(pbox[0], pbox[2])) - 0.01
        variants["c"] = _DeviceLayers([(polar, pbox, proj, gate, (-1.0,)), (glob, gbox, None, None, ())])
    torch.cuda.synchronize()
    plan = SG.SupergridPlan(inverse_resolution=a.res, ensure_nj_even=True)
    g = SG.Supergrid(plan, device="cuda:0")
    g.run_pass()
    cut = g.south_cut()
    halo = g.quality_halo(cut)
    if a.once:
        ms, recs = run(g, cut, halo, variants[a.once])
        print(json.dumps(dict(variant=a.once, ms=ms, **counts(recs))))
        return
    out = {"res": a.res, "arcsec": a.arcsec, "polar_m": a.polar_m, "nyp": g.stitched_rows(cut), "nxp": plan.Ni + 1,
           "global_raster": list(glob.shape), "polar_raster": list(variants["c"].tensors[0].shape)}
    first = {}
    for k in want:   # warm-up
        _, first[k] = run(g, cut, halo, variants[k])
        out[k] = counts(first[k])
    out["b_records_equal_a"] = all(bool((ra == rb[..., :7]).all()) for (_, _, ra), (_, _, rb) in zip(first["a"], first["b"]))
    del first
    times = {k: [] for k in want}
    for _ in range(a.reps):
        for k in want:
            ms, recs = run(g, cut, halo, variants[k])
            times[k].append(ms)
            del recs
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    for k in want:
        out[k].update(ms=times[k], ms_best=min(times[k]), ms_median=med(times[k]))
    ta, tb, tc = (med(times[k]) for k in want)
    ns_a, ns_b = ta * 1e6 / out["a"]["samples"], tb * 1e6 / out["b"]["samples"]
    n_polar, n_other = out["c"]["n_from"][0], out["c"]["samples"] - out["c"]["n_from"][0]
    out["derived"] = {"b_over_a_median": tb / ta, "b_over_a_best": min(times["b"]) / min(times["a"]), "ns_per_sample_a": ns_a,
                      "ns_per_sample_b": ns_b, "c_projected_samples": n_polar, "c_other_samples": n_other,
                      "ns_per_projected_sample": (tc * 1e6 - ns_b * n_other) / max(1, n_polar),
                      "projected_over_latlon": (tc * 1e6 - ns_b * n_other) / max(1, n_polar) / ns_b}
    print(json.dumps(out))
    if a.json:
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
