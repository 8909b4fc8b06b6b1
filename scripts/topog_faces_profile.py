"""Time face topography (csrc/ogg_topog.hip, topog_faces_kernel) beside the single-source topography kernel on a generated grid against
the synthetic global int16 raster of scripts/topog_profile.py, built on the device (nothing is downloaded).

    python scripts/topog_faces_profile.py [--res 8] [--arcsec 15] [--reps 5] [--refine R] [--json OUT]
    python scripts/topog_faces_profile.py --once u ...      (one run of one variant and nothing else: for a counter run)

After a warm-up of each, every repetition runs, one after the other in one process, so that all see the same box at the same time,
    (a) the topography kernel (ogg_topog_band_dev, model cells) over the whole stitched grid as one band,
    (u) the u faces alone (ogg_topog_faces_dev with an empty v range),
    (v) the v faces alone,
with HIP events around each call.  It reports the samples (n + n_missing over the records), the times and the ns per sample, and the
ratio the issue of the feature asks about: both families together per sample over (a) per sample (expected: about 1.3 or less).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))


def main(argv=None):
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--once", choices=("a", "u", "v"), default=None)
    p.add_argument("--res", type=float, default=8.0)
    p.add_argument("--arcsec", type=int, default=15)
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--refine", type=int, default=None)
    p.add_argument("--json", default=None)
    a = p.parse_args(argv)
    import torch

    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import face_topography as FT
    from ocean_model_grid_generator_amd import ocean_mask as M
    from ocean_model_grid_generator_amd import supergrid as SG
    from ocean_model_grid_generator_amd import topography as T
    from topog_profile import _DeviceRaster, synthetic_raster
    dev = torch.device("cuda:0")
    raster, box = synthetic_raster(a.arcsec, dev)
    src = _DeviceRaster(raster, box)
    plan = SG.SupergridPlan(inverse_resolution=a.res, ensure_nj_even=True)
    g = SG.Supergrid(plan, device="cuda:0")
    g.run_pass()
    x, y = g.stitched_xy(g.south_cut())
    nyp, nxp = x.shape
    ny, nx = nyp - 1, nxp - 1
    topology = M.topology_flags(*M.topology_of_device_grid(x, y))
    st = torch.cuda.current_stream(dev).cuda_stream
    band = L.TopogBand(nx=nx, j0=0, n_cell_rows=ny, cells=L.TOPOG_MODEL_CELLS, refine=int(a.refine or 0), oversample=2.0)
    band.x, band.y, band.x_next, band.y_next = x.data_ptr(), y.data_ptr(), x[ny].data_ptr(), y[ny].data_ptr()

    def faces(u_rows, v_rows):
        q = FT.params(ny, nx, topology, a.refine, 2.0, ld=x.stride(0), u_rows=u_rows, v_rows=v_rows, desc=src.desc, device=True)
        return q.points(x.data_ptr(), y.data_ptr())
    pu, pv = faces(None, (0, 0)), faces((0, 0), None)
    calls = {"a": lambda: T.band_records_dev(band, src.desc, st, dev)[1],
             "u": lambda: FT.records_dev(pu, src.desc, st, dev)[0],
             "v": lambda: FT.records_dev(pv, src.desc, st, dev)[1]}

    def run(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        t = calls[k]()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), t
    want = ("a", "u", "v") if not a.once else (a.once,)
    out = {"res": a.res, "arcsec": a.arcsec, "refine": a.refine, "nyp": nyp, "nxp": nxp, "raster": list(raster.shape), "topology": topology}
    for k in want:   # warm-up, and the samples
        ms, t = run(k)
        out[k] = {"records": int(t.shape[0] * t.shape[1]), "samples": int(t[..., 0].sum()) + int(t[..., 1].sum())}
        if a.once:
            out[k]["ms"] = ms
        del t
    if a.once:
        print(json.dumps(out))
        return
    times = {k: [] for k in want}
    for _ in range(a.reps):
        for k in want:
            ms, t = run(k)
            times[k].append(ms)
            del t
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    for k in want:
        out[k].update(ms=times[k], ms_best=min(times[k]), ms_median=med(times[k]), ns_per_sample=med(times[k]) * 1e6 / out[k]["samples"])
    both = (med(times["u"]) + med(times["v"])) * 1e6 / (out["u"]["samples"] + out["v"]["samples"])
    out["derived"] = {"faces_samples_over_topography": (out["u"]["samples"] + out["v"]["samples"]) / out["a"]["samples"],
                      "ns_per_sample_faces": both, "faces_over_topography_per_sample": both / out["a"]["ns_per_sample"],
                      "u_over_topography_per_sample": out["u"]["ns_per_sample"] / out["a"]["ns_per_sample"],
                      "v_over_topography_per_sample": out["v"]["ns_per_sample"] / out["a"]["ns_per_sample"]}
    print(json.dumps(out))
    if a.json:
        os.makedirs(os.path.dirname(os.path.abspath(a.json)), exist_ok=True)
        with open(a.json, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
