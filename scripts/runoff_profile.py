"""Time the runoff mapping (csrc/ogg_runoff.hip) at 1/8 degree with a synthetic 1/4-degree source (nothing is downloaded):

  cells       a regular 1/8-degree lat-lon supergrid of 2196 x 2880 model cells (periodic), with the generated-continent wet set of
              scripts/mask_profile.py (continents with ragged coasts, inland seas, lakes, islands and one-cell ponds)
  realistic   a 1440 x 720 float32 source with 12 records: discharge on the land source cells next to the coast and along a few
              "rivers" (lines of land cells running inland)
  worst       the same source non-zero on every land source cell

    python scripts/runoff_profile.py [--reps 20] [--json OUT] [--baseline]

For both cases: HIP-event medians of each step (targets, sources, search, segments, accumulate) over --reps runs after one warm-up
(the host's read of the counts between the sources and the search step is not timed), a torch fill of the accumulate step's output
bytes, and the brute-force search (OGG_RUNOFF_BRUTE=1, three runs).  --baseline adds the numpy definition's search on one host core,
timed on 2000 sources and scaled to all of them.
"""
import argparse
import ctypes
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

NY, NX = 2196, 2880
NA, NB, NREC = 1440, 720, 12


def grid(device):
    """supergrid x, y ((2 NY + 1) x (2 NX + 1)) and area (2 NY x 2 NX) of a regular grid from 80S to 90N, float64 device tensors"""
    import torch
    lon = torch.linspace(0.0, 360.0, 2 * NX + 1, dtype=torch.float64, device=device)
    lat = torch.linspace(-80.0, 90.0, 2 * NY + 1, dtype=torch.float64, device=device)
    y, x = torch.meshgrid(lat, lon, indexing="ij")
    s = torch.sin(torch.deg2rad(lat))
    area = (6371.0e3 ** 2) * torch.deg2rad(torch.diff(lon))[None, :] * torch.diff(s)[:, None]
    return x.contiguous(), y.contiguous(), area.contiguous()


def sources(wet, kind, device):
    """(NREC, NB, NA) float32 on the host: land source cells (those whose model cell is land) next to the coast and along a few rivers,
    or every land source cell"""
    import numpy as np
    w = wet.cpu().numpy().astype(bool)
    lon = (np.arange(NA) + 0.5) * 0.25
    lat = -90.0 + (np.arange(NB) + 0.5) * 0.25
    jj = np.clip(((lat + 80.0) / 170.0 * NY).astype(np.int64), 0, NY - 1)
    ii = np.clip((lon / 360.0 * NX).astype(np.int64), 0, NX - 1)
    land = ~w[jj[:, None], ii[None, :]] | (lat[:, None] < -80.0)
    if kind == "worst":
        pick = land
    else:
        near = np.zeros_like(land)
        wet_s = ~land
        for dj in (-1, 0, 1):
            for di in (-1, 0, 1):
                near |= np.roll(np.roll(wet_s, dj, axis=0), di, axis=1)
        pick = land & near
        rng = np.random.default_rng(5)
        for _ in range(40):   # rivers: random walks inland from a coastal land cell
            cj, ci = np.nonzero(pick)
            k = rng.integers(cj.size)
            j, i = cj[k], ci[k]
            for _ in range(200):
                j, i = int(np.clip(j + rng.integers(-1, 2), 0, NB - 1)), int((i + rng.integers(-1, 2)) % NA)
                if land[j, i]:
                    pick[j, i] = True
    rng = np.random.default_rng(6)
    f = (rng.random((NREC, NB, NA)) * 1e-3).astype(np.float32)
    return np.where(pick[None], f, np.float32(0.0)), int(pick.sum())


def ev():
    import torch
    return torch.cuda.Event(enable_timing=True)


def run(p, t, reps, brute=False):
    """per-step medians (ms)"""
    import torch
    from ocean_model_grid_generator_amd import _lib as L
    st = torch.cuda.current_stream().cuda_stream
    if brute:
        os.environ["OGG_RUNOFF_BRUTE"] = "1"
    rows = []
    for rep in range(reps + 1):
        e = [ev() for _ in range(6)]
        e[0].record()
        L.call("ogg_runoff_targets_dev", ctypes.byref(p), t["x"].data_ptr(), t["y"].data_ptr(), 2 * NX + 1, t["wet"].data_ptr(),
               t["ws"].data_ptr(), t["wsb"], t["tc"].data_ptr(), t["tu"].data_ptr(), t["counts"].data_ptr(), st)
        e[1].record()
        L.call("ogg_runoff_sources_dev", ctypes.byref(p), t["f"].data_ptr(), t["lon"].data_ptr(), t["lat"].data_ptr(), t["ws"].data_ptr(),
               t["wsb"], t["sc"].data_ptr(), t["su"].data_ptr(), t["ds"].data_ptr(), t["counts"].data_ptr(), st)
        e[2].record()
        c = t["counts"].cpu().tolist()
        nt, nm = c[0], c[1]
        e3 = ev()
        e3.record()
        L.call("ogg_runoff_search_dev", ctypes.byref(p), t["tc"].data_ptr(), t["tu"].data_ptr(), nt, t["su"].data_ptr(), nm, t["ws"].data_ptr(),
               t["wsb"], t["st"].data_ptr(), t["sd"].data_ptr(), t["counts"].data_ptr(), st)
        e[3].record()
        L.call("ogg_runoff_segments_dev", ctypes.byref(p), t["st"].data_ptr(), nm, t["ws"].data_ptr(), t["wsb"], st)
        e[4].record()
        L.call("ogg_runoff_accumulate_dev", ctypes.byref(p), t["f"].data_ptr(), t["sc"].data_ptr(), nm, t["area"].data_ptr(), 2 * NX,
               t["ws"].data_ptr(), t["wsb"], t["values"].data_ptr(), t["nsrc"].data_ptr(), t["counts"].data_ptr(), st)
        e[5].record()
        torch.cuda.synchronize()
        if rep:
            rows.append([e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), e3.elapsed_time(e[3]), e[3].elapsed_time(e[4]),
                         e[4].elapsed_time(e[5])])
    os.environ.pop("OGG_RUNOFF_BRUTE", None)
    med = [sorted(r[k] for r in rows)[len(rows) // 2] for k in range(5)]
    counts = dict(zip(L.RUNOFF_COUNT_FIELDS, t["counts"].cpu().tolist()))
    return dict(zip(("targets_ms", "sources_ms", "search_ms", "segments_ms", "accumulate_ms"), med)), counts


def fill_ms(values, reps):
    import torch
    out = []
    for _ in range(reps + 1):
        a, b = ev(), ev()
        a.record()
        values.fill_(0.0)
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return sorted(out[1:])[reps // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", default=None)
    ap.add_argument("--baseline", action="store_true")
    a = ap.parse_args()
    import numpy as np
    import torch

    from mask_profile import wet_set
    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import remap as R
    from ocean_model_grid_generator_amd import runoff as RO
    dev = "cuda:0"
    x, y, area = grid(dev)
    wet = (wet_set("realistic", NY, NX, dev) > 0).to(torch.uint8).contiguous()
    lon_e = np.linspace(0.0, 360.0, NA + 1)
    lat_e = np.linspace(-90.0, 90.0, NB + 1)
    rows = []
    for kind in ("realistic", "worst"):
        f, npick = sources(wet, kind, dev)
        src = R.Source(f, lon_e, lat_e)
        p = RO.params(NY, NX, src, "coast", True, False)
        wsb = int(L.load().ogg_runoff_workspace_bytes(ctypes.byref(p)))
        nc, ns = NY * NX, NA * NB
        t = dict(x=x, y=y, area=area, wet=wet, wsb=wsb, ws=torch.empty(wsb, dtype=torch.uint8, device=dev),
                 f=torch.from_numpy(f).to(dev), lon=torch.from_numpy(lon_e).to(dev), lat=torch.from_numpy(lat_e).to(dev),
                 tc=torch.empty(nc, dtype=torch.int32, device=dev), tu=torch.empty((nc, 3), dtype=torch.float64, device=dev),
                 sc=torch.empty(ns, dtype=torch.int32, device=dev), su=torch.empty((ns, 3), dtype=torch.float64, device=dev),
                 ds=torch.empty(NB, dtype=torch.float64, device=dev), st=torch.empty(ns, dtype=torch.int32, device=dev),
                 sd=torch.empty(ns, dtype=torch.float64, device=dev),
                 values=torch.empty((NREC, NY, NX), dtype=torch.float64, device=dev),
                 nsrc=torch.empty((NY, NX), dtype=torch.int32, device=dev),
                 counts=torch.zeros(len(L.RUNOFF_COUNT_FIELDS), dtype=torch.int64, device=dev))
        steps, counts = run(p, t, a.reps)
        keep = {k: t[k].clone() for k in ("st", "sd", "values")}
        brute, bc = run(p, t, 3, brute=True)
        same = all(torch.equal(keep[k][: counts["mapped"]], t[k][: counts["mapped"]]) for k in ("st", "sd")) and \
            torch.equal(keep["values"], t["values"])
        fill = fill_ms(t["values"], a.reps)
        row = dict(case=kind, shape=[NY, NX], source=[NB, NA], records=NREC, **steps, fill_ms=fill,
                   accumulate_over_fill=steps["accumulate_ms"] / fill, brute_search_ms=brute["search_ms"], brute_tests=bc["tests"],
                   brute_equal=bool(same), total_ms=sum(steps.values()), **counts)
        print(json.dumps(row))
        rows.append(row)
        if a.baseline and kind == "realistic":
            import runoff_definition as D
            nt, nm = counts["targets"], counts["mapped"]
            tu, su = t["tu"][:nt].cpu().numpy(), t["su"][:nm].cpu().numpy()
            tcell = t["tc"][:nt].cpu().numpy()
            k = min(2000, nm)
            t0 = time.perf_counter()
            D.nearest(su[:k], tu, tcell)
            dt = time.perf_counter() - t0
            row = {"case": kind, "numpy_definition_search_s_scaled": dt * nm / k, "timed_sources": k, "sources": nm, "targets": nt}
            print(json.dumps(row))
            rows.append(row)
    if len(rows) >= 2:
        r, w = rows[0], next(q for q in rows if q.get("case") == "worst" and "total_ms" in q)
        print(json.dumps({"worst_over_realistic": w["total_ms"] / r["total_ms"]}))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": L.device_name(), "library": L.load().ogg_version().decode(), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
