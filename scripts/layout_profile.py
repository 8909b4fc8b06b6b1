"""Time the processor-layout kernels (csrc/ogg_layout.hip) on one GPU (nothing is downloaded), on the cases of the coast-distance
profile (scripts/coast_distance_profile.py): om4, the generated 1/4-degree OM4 tripolar grid with the synthetic continents of the
tests, and r8, a regular 1/8-degree grid of 2196 x 2880 model cells with the generated-continent wet set of scripts/mask_profile.py.

    python scripts/layout_profile.py [--cases om4 r8] [--reps 20] [--sweep_reps 5] [--host_subset 150] [--json OUT]

For every case: HIP-event times of the table build (ogg_layout_table_dev) over --reps runs after one warm-up, against a torch fill
of the table's bytes in the same process; the sweep (ogg_layout_sweep_dev) for max_blocks 4096 and 16384 (min_block 2; the candidate
counts are printed) with halo 0 and halo 4, over --sweep_reps runs; and a numpy host baseline that also works from a summed-area
table (vectorised over the blocks of a layout, the extents from ogg_layout_extent), timed on one core on a random subset of
--host_subset candidates, checked against the device's masked counts and scaled to the whole list by the candidate count.  Last, 1000 copies each of
three layouts of 16384 blocks (2048 x 8, 128 x 128, 8 x 2048) at halo 0: the blocks are as many, so the difference is the serial walk of
the extent rule by one lane per axis.
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


def ev():
    import torch
    return torch.cuda.Event(enable_timing=True)


def stats(v):
    v = sorted(v)
    return {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}


def timed(fn, reps):
    import torch
    out = []
    for _ in range(reps + 1):
        a, b = ev(), ev()
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b))
    return stats(out[1:])


# ---- the numpy baseline ------------------------------------------------------------------------------------------------
def host_masked(S, ny, nx, periodic, fold, h, bx, ex, by, ey):
    """the masked count of one layout from the summed-area table S with numpy, vectorised over its blocks (rectangles may overlap:
    only count == 0 is asked)"""
    import numpy as np

    def rect(r0, r1, c0, c1):   # (rows, cols) outer product of inclusive ranges; empty ranges give 0
        v = S[np.ix_(r1 + 1, c1 + 1)] - S[np.ix_(r0, c1 + 1)] - S[np.ix_(r1 + 1, c0)] + S[np.ix_(r0, c0)]
        return np.where((r1 >= r0)[:, None] & (c1 >= c0)[None, :], v, 0)
    if h == 0:
        return int((rect(by, ey, bx, ex) == 0).sum())
    r0, r1 = np.maximum(by - h, 0), np.minimum(ey + h, ny - 1)
    cl, cr = bx - h, ex + h
    if periodic:
        wide = cr - cl + 1 >= nx
        l, r = cl % nx, cr % nx
        split = ~wide & (l > r)
        cols = [(np.where(wide, 0, l), np.where(wide, nx - 1, np.where(split, nx - 1, r))), (np.zeros_like(l), np.where(split, r, -1))]
    else:
        cols = [(np.maximum(cl, 0), np.minimum(cr, nx - 1))]
    n = sum(rect(r0, r1, c0, c1) for c0, c1 in cols)
    if fold:
        past = ey + h - ny
        f0 = np.where(past >= 0, np.maximum(ny - 1 - past, 0), ny)   # an empty range where the halo stays below the fold
        f1 = np.full_like(f0, ny - 1)
        n = n + sum(rect(np.minimum(f0, ny - 1), np.where(past >= 0, f1, -1), np.maximum(nx - 1 - c1, 0), np.where(c1 >= c0, nx - 1 - c0, -1))
                    for c0, c1 in cols)
    return int((n == 0).sum())


def host_baseline(LY, wet, periodic, fold, h, cand, subset, seed=0):
    """(seconds for the subset, table seconds, the subset's indices, its masked counts)"""
    import numpy as np
    ny, nx = wet.shape
    t0 = time.perf_counter()
    S = np.zeros((ny + 1, nx + 1), np.int64)
    S[1:, 1:] = np.cumsum(np.cumsum(wet != 0, axis=0, dtype=np.int64), axis=1)
    t_table = time.perf_counter() - t0
    idx = np.sort(np.random.default_rng(seed).choice(cand.shape[0], size=min(subset, cand.shape[0]), replace=False))
    masked = []
    t0 = time.perf_counter()
    for k in idx:
        bx, ex = (v.astype(np.int64) for v in LY.extent(nx, int(cand["px"][k])))
        by, ey = (v.astype(np.int64) for v in LY.extent(ny, int(cand["py"][k])))
        masked.append(host_masked(S, ny, nx, periodic, fold, h, bx, ex, by, ey))
    return time.perf_counter() - t0, t_table, idx, np.array(masked)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", default=["om4", "r8"], choices=["r2", "om4", "r8"])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--sweep_reps", type=int, default=5)
    ap.add_argument("--host_subset", type=int, default=150)
    ap.add_argument("--max_blocks", type=int, nargs="+", default=[4096, 16384])
    ap.add_argument("--halos", type=int, nargs="+", default=[0, 4])
    ap.add_argument("--json", default=None)
    a = ap.parse_args()
    os.environ.setdefault("OMP_NUM_THREADS", "1")
    import numpy as np
    import torch

    from coast_distance_profile import case_grid
    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import layout as LY
    torch.set_num_threads(1)
    dev = "cuda:0"
    rows = []
    for name in a.cases:
        _, _, wet, periodic, fold = case_grid(name, dev)
        ny, nx = (int(v) for v in wet.shape)
        hwet = wet.cpu().numpy()
        t = LY.DeviceTable(wet, periodic, fold, 0)
        st = torch.cuda.current_stream().cuda_stream
        build = timed(lambda: L.call("ogg_layout_table_dev", ctypes.byref(t.p), t.wet.data_ptr(), t.ws.data_ptr(), t.wsb, st), a.reps)
        out = torch.empty((ny + 1) * (nx + 1), dtype=torch.int32, device=dev)
        fill = timed(lambda: out.fill_(0), a.reps)
        row = dict(case=name, shape=[ny, nx], periodic=bool(periodic), fold=bool(fold), wet=int(hwet.sum()), table_ms=build, fill_ms=fill,
                   table_over_fill=build["median"] / fill["median"], sweeps=[])
        for mb in a.max_blocks:
            t0 = time.perf_counter()
            cand = LY.sweep_candidates(ny, nx, mb, 2)
            t_cand = time.perf_counter() - t0
            dc = torch.from_numpy(cand.view(np.int32).reshape(-1, 2)).to(dev)
            dr = torch.empty((cand.shape[0], len(L.LAYOUT_RECORD_FIELDS)), dtype=torch.int32, device=dev)
            for h in a.halos:
                th = LY.DeviceTable(wet, periodic, fold, h)
                ms = timed(lambda: L.call("ogg_layout_sweep_dev", ctypes.byref(th.p), dc.data_ptr(), cand.shape[0], th.ws.data_ptr(), th.wsb,
                                          dr.data_ptr(), st), a.sweep_reps)
                rec = np.ascontiguousarray(dr.cpu().numpy()).view(L.LAYOUT_RECORD).reshape(-1)
                sec, t_table, idx, masked = host_baseline(LY, hwet, periodic, fold, h, cand, a.host_subset)
                scaled = sec * cand.shape[0] / idx.size
                row["sweeps"].append(dict(max_blocks=mb, halo=h, candidates=int(cand.shape[0]), blocks_total=int(rec["blocks"].astype(np.int64).sum()),
                                          candidates_s=t_cand, sweep_ms=ms, host_subset=int(idx.size), host_subset_s=sec, host_table_s=t_table,
                                          host_scaled_s=scaled, host_over_device=scaled * 1000.0 / ms["median"],
                                          host_equal=bool(np.array_equal(masked, rec["masked"][idx])),
                                          usable=int((rec["status"] == 0).sum()), masked_max=int(rec["masked"].max())))
                del th
        # the serial share: 1000 copies each of three layouts of 16384 blocks whose rule walks 2048 + 8, 128 + 128 and 8 + 2048 steps
        row["shape_probe"] = []
        for px, py in ((2048, 8), (128, 128), (8, 2048)):
            if px > nx or py > ny:
                continue
            pc = torch.tensor([[px, py]] * 1000, dtype=torch.int32, device=dev)
            pr = torch.empty((1000, len(L.LAYOUT_RECORD_FIELDS)), dtype=torch.int32, device=dev)
            ms = timed(lambda: L.call("ogg_layout_sweep_dev", ctypes.byref(t.p), pc.data_ptr(), 1000, t.ws.data_ptr(), t.wsb, pr.data_ptr(), st),
                       a.sweep_reps)
            row["shape_probe"].append(dict(px=px, py=py, copies=1000, sweep_ms=ms))
        print(json.dumps(row), flush=True)
        rows.append(row)
        del t
        torch.cuda.empty_cache()
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"device": L.device_name(), "library": L.load().ogg_version().decode(), "rows": rows}, fh, indent=1)


if __name__ == "__main__":
    main()
