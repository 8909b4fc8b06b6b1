"""Do two builds of libogg_hip.so give the cell-set analyses the same bytes?  Runoff, coast distance (both sides), basin codes, the
ocean mask (with and without seeds) and the remap fill on every shape and cut of tests/small_meshes.py and on the generated 1-degree
tripolar grid with the continents of tests/test_gpu_runoff.py, once with default knobs and once with the brute-force knobs; the
sha256 of every output array and every field of every counts struct, one fresh child process per library and knob set (one GPU):

    python scripts/analyses_ab.py ab/libogg_hip_parent.so ocean_model_grid_generator_amd/csrc/libogg_hip.so > profiles/<name>.md
"""
import hashlib
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
KNOBS = {"default": {}, "brute": {"OGG_RUNOFF_BRUTE": "1", "OGG_COAST_BRUTE": "1", "OGG_BASIN_BATCH": "0"}}
FULL = (-180.0, 180.0, -90.0, 90.0)


def sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()   # tobytes() is the C-order copy


def show(tag, res, keys):
    """one line per array of res (a dict) under ``keys``, one for its counts; an exception's text stands for the outputs"""
    if isinstance(res, Exception):
        return print(tag, "refused:", res)
    for k in keys:
        print(tag, k, sha(res[k]))
    c = res.get("counts") or res["summary"]
    print(tag, "counts", " ".join("%s=%s" % (k, c[k]) for k in sorted(c) if isinstance(c[k], int)))


def attempt(fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except Exception as e:   # a refusal is part of the listing: both builds must give the same one
        return e


def child():
    import numpy as np
    import torch
    import small_meshes as SM
    from test_gpu_remap import device_grid
    from test_gpu_runoff import wet_of
    from ocean_model_grid_generator_amd import _lib as L, basin_codes as BC, coast_distance as CD, ocean_mask as M, remap as R, runoff as RO
    import ocean_model_grid_generator_amd.supergrid as sg
    grids = {n: SM.shape_grid(n) for n in SM.SHAPES}
    grids.update(("cut_" + n, g) for n, g in SM.topology_cuts().items())
    plan, ranks = device_grid(sg, "r1")
    grids["r1"] = sg.stitch(plan, [ranks[0].bands_to_host()])
    dev = torch.device("cuda:0")
    for name, g in grids.items():
        x, y, area = g["x"], g["y"], g["area"]
        ny, nx = (x.shape[0] - 1) // 2, (x.shape[1] - 1) // 2
        wet = wet_of(x, y) if name == "r1" else SM.wet_mask(ny, nx)
        cen = lambda j, i: (float(x[2 * j + 1, 2 * i + 1]), float(y[2 * j + 1, 2 * i + 1]))   # noqa: E731
        f, lon, lat, fills = SM.source_for(x, y, "regular", nrec=2, dtype=np.float32)
        show(name + " runoff", attempt(RO.runoff, x, y, area, R.Source(np.abs(f), lon, lat, fill=fills), wet),
             ("values", "n_sources", "src_cell", "src_target", "src_d2"))
        show(name + " coast", attempt(CD.coast_distance, x, y, wet, "both"), ("nearest", "d2", "flags"))
        rules = [(1,) + cen(0, 0) + FULL, (2,) + cen(ny - 1, nx - 1) + FULL, (3,) + cen(ny // 2, nx // 2) + FULL]
        show(name + " basin", attempt(BC.basin_codes, x, y, wet, rules), ("code", "rule", "records"))
        depth = np.where(wet != 0, 50.0 + 40.0 * np.cos(np.arange(ny * nx).reshape(ny, nx)), 0.0)
        j, i = np.argwhere(depth >= 20.0)[-1]   # the seed: the last cell that stays wet
        for tag, seeds in (("mask", ()), ("mask_seeded", [cen(int(j), int(i))])):
            show(name + " " + tag, attempt(M.ocean_mask, depth, x, y, min_depth=20.0, seeds=seeds), ("depth", "wet", "root"))
        v, fl = SM.synthetic_flags(ny, nx, 3, 11 * ny + nx)
        src = R.Source(np.zeros((3, 2, 3)), *SM.source_edges("3x2"))
        for periodic, fold in ((False, False), (True, True)):
            tv = torch.from_numpy(np.ascontiguousarray(v)).to(dev)
            tf = R.flags_buffer(torch, tv.numel(), dev).view(v.shape)
            tf.copy_(torch.from_numpy(fl))
            ct = torch.zeros(len(L.REMAP_COUNT_FIELDS), dtype=torch.int64, device=dev)
            R.fill_dev(R.params(ny, nx, src, 0, periodic, fold, None), tv, tf, ct, torch.cuda.current_stream(dev).cuda_stream, dev)
            show("%s fill_%d%d" % (name, periodic, fold), {"values": tv.cpu().numpy(), "flags": tf.cpu().numpy(),
                                                          "counts": R.counts_dict(ct.cpu().numpy())}, ("values", "flags"))


def main(libs):
    listings = []
    for lib in libs:
        text = ""
        for knobs, env in KNOBS.items():
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"], env=dict(os.environ, OGG_LIB_PATH=os.path.abspath(lib), **env),
                               stdout=subprocess.PIPE, text=True, timeout=900)
            if r.returncode != 0:   # nothing more is started on the GPU after a child that failed
                sys.exit("%s (%s knobs) ended with status %d" % (lib, knobs, r.returncode))
            text += "".join("%s: %s\n" % (knobs, line) for line in r.stdout.splitlines())
        listings.append(text)
    same = all(t == listings[0] for t in listings)
    print("# The analyses' bytes under %s\n\n%s: %d lines per library.\n\n```\n%s```"
          % (" and ".join(os.path.basename(p) for p in libs), "IDENTICAL listings" if same else "THE LISTINGS DIFFER", listings[0].count("\n"), listings[0]))
    if not same:
        print("\n".join("```\n%s```" % t for t in listings[1:]))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(child() if "--child" in sys.argv else main(sys.argv[1:]))
