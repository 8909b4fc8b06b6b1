"""The regional grids on the device (csrc/ogg_regional.hip) against the 50-digit truth (tests/golden/regional_truth.npz), against
themselves under every split into bands and through their three entries, and through the command into the existing analyses.

Shapes: those of tests/regional_definition.py (CASES): 2 x 2 supergrid cells, 130 x 2 and 2 x 130, point rows of 63, 65 and 129 around
a wavefront's 64 lanes (nx is even, so a row of 64 is the dx and area row of nx = 64), 8 x 8 next to the pole, 258 x 10 (two workgroups
across a row, two row chunks).

Measured on an MI355X (the first test prints them), largest distance from the truth, device / fp64 definition:
    away from the poles   x 3.15e-14 / 3.15e-14 deg   y 2.43e-14 / 1.92e-14 deg   angle_dx 3.60e-14 / 3.31e-14 deg
                          dx 3.02e-16 / 3.02e-16      dy 1.70e-16 / 2.08e-14      area 3.82e-16 / 1.55e-14   (relative)
    lat_c = 89            x 1.19e-13 / 1.19e-13 deg   y 1.93e-14 / 1.42e-14 deg   angle_dx 1.25e-13 / 1.29e-13 deg
                          dx 1.38e-16 / 1.31e-16      dy 1.48e-16 / 2.21e-16      area 2.56e-16 / 3.02e-16   (relative)
(dy and area: the device forms the row differences without cancellation, the definition literally.)
"""
import itertools
import json
import os

import numpy as np
import pytest

import regional_definition as rd

pytestmark = pytest.mark.gpu
K_REF = 1.5        # the project's rule (tests/test_gpu_truth.py)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regional_truth.npz")
SHAPES = [(2, 2), (130, 2), (2, 130), (62, 4), (64, 4), (128, 4), (258, 10)]     # (nx, ny)


@pytest.fixture(scope="module")
def R(hip):
    from ocean_model_grid_generator_amd import regional
    return regional


@pytest.fixture(scope="module")
def truth():
    return np.load(GOLDEN)


def host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def same_bytes(a, b, names=rd.FIELDS):
    return [n for n in names if a[n].shape != b[n].shape or a[n].tobytes() != b[n].tobytes()]


def test_device_against_the_truth(R, truth, capsys):
    """Per field, the device's largest distance from the truth is at most 1.5 times the fp64 definition's own (as recorded with the
    truth) over the same points.  The points are taken in two groups, each held to the rule on its own: the cases with lat_c = 89,
    where x and angle_dx are ill-conditioned (an error of the unit vector is divided by the distance from the pole) and would hide every
    other case behind their errors, and the rest.  Where the definition's error is exactly zero for a whole field of a case (the
    untilted grids at the equator: x = lon_c + lam', y = phi' in whole steps, angle_dx = 0; angle_dx = -180 with tilt = -180) 1.5 times
    nothing is no bound: the device must give the definition's bits there."""
    eref = truth["eref"]
    dev_err = np.zeros((len(rd.CASES), len(rd.FIELDS)))
    not_exact = []
    for k, case in enumerate(rd.CASES):
        got = host(R.regional_grid_dev(**rd.case_args(case)))
        ref = rd.regional(**rd.case_args(case))
        for f, name in enumerate(rd.FIELDS):
            hi, lo = truth["%s/%s" % (case[0], name)]
            assert got[name].shape == hi.shape and np.all(np.isfinite(got[name])), (case[0], name)
            dev_err[k, f] = rd.error(name, got[name], hi, lo).max()
            if eref[k, f] == 0.0 and rd.error(name, ref[name], hi, lo).max() == 0.0:
                bad = got[name].view(np.int64) != ref[name].view(np.int64)
                if bad.any():
                    not_exact.append((case[0], name, int(bad.sum()), bad.size))
    groups = {"lat_c = 89": [k for k, c in enumerate(rd.CASES) if c[0] in rd.POLAR], "away from the poles": [k for k, c in enumerate(rd.CASES) if c[0] not in rd.POLAR]}
    with capsys.disabled():
        print()
        for k, case in enumerate(rd.CASES):
            print("regional vs truth %-20s %s" % (case[0], "  ".join("%s %.2e/%.2e" % (n, dev_err[k, f], eref[k, f]) for f, n in enumerate(rd.FIELDS))))
        for g, ks in groups.items():
            print("regional vs truth, %s: device / definition  %s" % (g, "  ".join("%s %.3e / %.3e" % (n, dev_err[ks, f].max(), eref[ks, f].max())
                                                                                     for f, n in enumerate(rd.FIELDS))))
    assert not_exact == []
    zero = {(c[0], n) for k, c in enumerate(rd.CASES) for f, n in enumerate(rd.FIELDS) if eref[k, f] == 0.0}
    assert zero >= {("2x2_origin", "y"), ("2x2_origin", "angle_dx"), ("130x2_equator", "x"), ("62x4_plain", "x"), ("128x4_flipped", "angle_dx")}
    for g, ks in groups.items():
        for f, name in enumerate(rd.FIELDS):
            assert eref[ks, f].max() > 0.0
            assert dev_err[ks, f].max() <= K_REF * eref[ks, f].max(), (g, name, dev_err[ks, f].max(), eref[ks, f].max())


def run_bands(R, L, p, rows, metrics=True):
    """the band entry called with the given [(first point row, point rows)], each band into the rows of whole-grid tensors"""
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    wsb = int(L.load().ogg_regional_workspace_bytes(*p))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    names = rd.FIELDS if metrics else rd.FIELDS[:2]
    out = {f: torch.full(R.shapes(p.nx, p.ny)[f], float("nan"), dtype=torch.float64, device=dev) for f in names}
    L.call("ogg_regional_tables_dev", *(list(p) + [ws.data_ptr(), wsb, st]))
    for j0, n in rows:
        ptrs = [(out[f][j0:].data_ptr() if j0 < out[f].shape[0] else None) if f in out else None for f in rd.FIELDS]
        L.call("ogg_regional_band_dev", *(list(p) + [j0, n, ws.data_ptr(), wsb] + ptrs + [st]))
    return host(out)


@pytest.mark.parametrize("kind", ["latlon", "mercator"])
def test_every_split_into_bands(R, hip, kind):
    """A grid of 9 point rows: every split into one, two and three bands (1 + 8 + 28), in either order of the launches, gives the
    whole grid's bytes; without metrics the same x and y bytes and nothing else."""
    args = dict(lon_c=-64.5, lat_c=52.0, nx=66, ny=8, delta=0.125, kind=kind, tilt=-17.0)
    p = R.params(**args)
    whole = run_bands(R, hip, p, [(0, 9)])
    assert all(np.all(np.isfinite(whole[f])) for f in rd.FIELDS)
    splits = [c for n in (1, 2) for c in itertools.combinations(range(1, 9), n)]
    assert len(splits) == 8 + 28
    for cuts in splits:
        edges = (0,) + cuts + (9,)
        rows = [(a, b - a) for a, b in zip(edges[:-1], edges[1:])]
        assert same_bytes(whole, run_bands(R, hip, p, rows)) == [], cuts
        assert same_bytes(whole, run_bands(R, hip, p, rows[::-1])) == [], cuts
    p0 = R.params(metrics=False, **args)
    for rows in ([(0, 9)], [(0, 4), (4, 5)], [(0, 1), (1, 7), (8, 1)]):
        xy = run_bands(R, hip, p0, rows, metrics=False)
        assert sorted(xy) == ["x", "y"] and same_bytes(whole, xy, ("x", "y")) == []


@pytest.mark.parametrize("nx, ny", SHAPES)
def test_the_three_entries_give_the_same_bytes(R, nx, ny):
    """the host-pointer entry (regional_grid), the device entries in one band and in three (regional_grid_dev), with and without
    metrics"""
    for kind, lat_c, tilt in (("mercator", 47.0, 25.0), ("latlon", -30.0, -100.0)):
        args = dict(lon_c=179.9, lat_c=lat_c, nx=nx, ny=ny, delta=0.125, kind=kind, tilt=tilt)
        a = R.regional_grid(**args)
        assert sorted(a) == sorted(rd.FIELDS) and all(a[f].shape == R.shapes(nx, ny)[f] for f in rd.FIELDS)
        assert same_bytes(a, host(R.regional_grid_dev(**args))) == []
        assert same_bytes(a, host(R.regional_grid_dev(bands=3, **args))) == []
        b = R.regional_grid(metrics=False, **args)
        assert sorted(b) == ["x", "y"] and same_bytes(a, b, ("x", "y")) == []
        assert same_bytes(a, host(R.regional_grid_dev(metrics=False, bands=2, **args)), ("x", "y")) == []
        ref = rd.regional(Re=rd.RE, **args)
        for f in rd.FIELDS:       # not the truth test: a gross check that the shapes above hold the right grid
            scale = np.abs(ref[f]).max()
            assert np.max(np.abs(a[f] - ref[f])) <= 1e-11 * max(scale, 1.0), f


COMMAND = ["--lon_c", "-52.25", "--lat_c", "61.5", "--tilt", "33.0", "-r", "4", "--cells", "12", "10", "--kind", "mercator", "--no_changing_meta"]


def test_round_trip_through_the_analyses(R, tmp_path, capsys):
    """A 12 x 10-cell tilted Mercator grid written by the command, read back: locate() puts every cell centre into its own cell with a
    positive margin; grid_quality reports no seam and the smallest dx the summary printed."""
    from ocean_model_grid_generator_amd import locate as LOC
    from ocean_model_grid_generator_amd import netcdf3
    path, q = str(tmp_path / "ocean_hgrid.nc"), str(tmp_path / "q.json")
    s = R.main(COMMAND + ["-f", path, "--quality_report", q])
    printed = capsys.readouterr().out
    g = netcdf3.read_doubles(path, names=("x", "y", "dx", "dy", "area", "angle_dx"))
    assert g["x"].shape == (21, 25) and g["dx"].shape == (21, 24) and g["dy"].shape == (20, 25) and g["area"].shape == (20, 24)
    direct = R.regional_grid(-52.25, 61.5, 24, 20, 0.125, "mercator", tilt=33.0)
    assert same_bytes(direct, g) == []
    assert abs(g["x"][10, 12] - -52.25) < 1e-12 and abs(g["y"][10, 12] - 61.5) < 1e-12 and abs(g["angle_dx"][10, 12] - 33.0) < 1e-12
    res = LOC.locate(g["x"], g["y"], g["x"][1::2, 1::2], g["y"][1::2, 1::2])
    assert np.array_equal(res["cell"], np.arange(120)) and np.all(res["margin"] > 0.0)
    assert not res["periodic"] and not res["fold"]
    rep = json.load(open(q))
    assert rep.get("joints", []) == []
    assert rep["grid"]["dx"]["min"]["value"] == s["dx_min"] == g["dx"].min()
    assert ("dx %.9g .. " % s["dx_min"]) in printed and "corners (lon, lat) SW" in printed and "closed form" in printed
    assert abs(s["area_relative_error"]) <= np.finfo(np.float64).eps * (24 * 20 + 16)      # a sum of nx ny rounded terms
    atts = netcdf3.read_header(path).gatts
    assert float(atts["regional_lon_c"][0]) == -52.25 and float(atts["regional_lat_c"][0]) == 61.5 and float(atts["regional_tilt"][0]) == 33.0
    assert atts["grid_kind"] == "regional mercator"


def test_the_file_is_reproducible(R, tmp_path, capsys):
    """with --no_changing_meta the file is byte-identical between two runs and between one band and three; --skip_metrics keeps the x and y bytes"""
    files = {}
    for name, extra in (("a", []), ("b", []), ("three", ["--bands", "3"])):
        files[name] = str(tmp_path / (name + ".nc"))
        R.main(COMMAND + ["-f", files[name]] + extra)
    first = open(files["a"], "rb").read()
    assert open(files["b"], "rb").read() == first and open(files["three"], "rb").read() == first
    assert b"regional_tilt" in first and b"history" not in first
    from ocean_model_grid_generator_amd import netcdf3
    skipped = str(tmp_path / "skip.nc")
    R.main(COMMAND + ["-f", skipped, "--skip_metrics"])
    a, b = (netcdf3.read_doubles(f, names=("x", "y", "dx")) for f in (files["a"], skipped))
    assert same_bytes(a, b, ("x", "y")) == [] and np.all(b["dx"] == -1.0)
    capsys.readouterr()
