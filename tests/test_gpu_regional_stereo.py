"""The stereographic regional grids on the device (csrc/ogg_regional_stereo.hip) against the 50-digit truth
(tests/golden/regional_stereo_truth.npz), against themselves under every split into bands and through their three entries, and
through the command into the existing analyses with a pole in the domain.

Shapes: those of tests/regional_stereo_definition.py (CASES): 2 x 2 supergrid cells, 130 x 2 and 2 x 130, point rows of 63, 65 and 129
around the 63 columns a wavefront owns and its 64 lanes, 258 x 10 (two workgroups across a row, two row chunks), and the polar cases.

Measured on an MI355X (the first test prints them), largest distance from the truth, device / fp64 definition:
    away from the poles   x 4.21e-14 / 4.21e-14 deg   y 2.45e-14 / 2.14e-14 deg   angle_dx 3.41e-14 / 4.40e-14 deg
                          dx 4.82e-16 / 6.58e-16      dy 4.63e-16 / 6.14e-16      area 5.56e-16 / 4.66e-14   (relative)
    the polar cases       x 2.27e-13 / 3.24e-12 deg   y 1.30e-14 / 1.57e-14 deg   angle_dx 2.43e-13 / 3.21e-12 deg
                          dx 4.18e-16 / 5.12e-16      dy 4.18e-16 / 5.12e-16      area 5.51e-16 / 1.80e-15   (relative)
(area: the device takes the definition's differences of neighbouring edges apart, the definition evaluates them literally; x and
angle_dx about a pole: the device takes the cosine of lat_c = +-90 as 0, the definition as the cosine of pi/2 rounded.)
"""
import itertools
import os

import numpy as np
import pytest

import regional_stereo_definition as sd

pytestmark = pytest.mark.gpu
K_REF = 1.5        # the project's rule (tests/test_gpu_truth.py)
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "regional_stereo_truth.npz")
SHAPES = [(2, 2), (130, 2), (2, 130), (62, 4), (64, 6), (128, 4), (258, 10)]     # (nx, ny)


@pytest.fixture(scope="module")
def S(hip):
    from ocean_model_grid_generator_amd import regional_stereo
    return regional_stereo


@pytest.fixture(scope="module")
def truth():
    return np.load(GOLDEN)


def host(d):
    return {k: v.cpu().numpy() for k, v in d.items()}


def same_bytes(a, b, names=sd.FIELDS):
    return [n for n in names if a[n].shape != b[n].shape or a[n].tobytes() != b[n].tobytes()]


def test_device_against_the_truth(S, truth, capsys):
    """Per field, the device's largest distance from the truth is at most 1.5 times the fp64 definition's own (as recorded with the
    truth) over the same points.  The points are taken in two groups, each held to the rule on its own: the polar cases (lat_c = +-90 and
    89.97), where x and angle_dx are ill-conditioned (an error of the unit vector is divided by the distance from the pole) and would
    hide every other case behind their errors, and the rest.  The one point that IS a pole has its three defined values, bit for bit."""
    eref = truth["eref"]
    dev_err = np.zeros((len(sd.CASES), len(sd.FIELDS)))
    for k, case in enumerate(sd.CASES):
        got = host(S.stereo_grid_dev(**sd.case_args(case)))
        name, lon_c, lat_c, tilt, delta, nx, ny = case
        if abs(lat_c) == 90.0:
            assert (got["x"][ny // 2, nx // 2], got["y"][ny // 2, nx // 2], got["angle_dx"][ny // 2, nx // 2]) == (lon_c, lat_c, tilt), name
        for f, field in enumerate(sd.FIELDS):
            hi, lo = truth["%s/%s" % (name, field)]
            assert got[field].shape == hi.shape and np.all(np.isfinite(got[field])), (name, field)
            dev_err[k, f] = sd.error(field, got[field], hi, lo).max()
    groups = {"polar": [k for k, c in enumerate(sd.CASES) if c[0] in sd.POLAR], "away from the poles": [k for k, c in enumerate(sd.CASES) if c[0] not in sd.POLAR]}
    with capsys.disabled():
        print()
        for k, case in enumerate(sd.CASES):
            print("stereo vs truth %-16s %s" % (case[0], "  ".join("%s %.2e/%.2e" % (n, dev_err[k, f], eref[k, f]) for f, n in enumerate(sd.FIELDS))))
        for g, ks in groups.items():
            print("stereo vs truth, %s: device / definition  %s" % (g, "  ".join("%s %.3e / %.3e" % (n, dev_err[ks, f].max(), eref[ks, f].max())
                                                                                   for f, n in enumerate(sd.FIELDS))))
    for g, ks in groups.items():
        assert len(ks) >= 4
        for f, field in enumerate(sd.FIELDS):
            assert eref[ks, f].max() > 0.0
            assert dev_err[ks, f].max() <= K_REF * eref[ks, f].max(), (g, field, dev_err[ks, f].max(), eref[ks, f].max())


def run_bands(S, L, p, rows, metrics=True):
    """the band entry called with the given [(first point row, point rows)], each band into the rows of whole-grid tensors"""
    import torch
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream(dev).cuda_stream
    wsb = int(L.load().ogg_regional_stereo_workspace_bytes(*p))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    names = sd.FIELDS if metrics else sd.FIELDS[:2]
    out = {f: torch.full(S.shapes(p.nx, p.ny)[f], float("nan"), dtype=torch.float64, device=dev) for f in names}
    L.call("ogg_regional_stereo_tables_dev", *(list(p) + [ws.data_ptr(), wsb, st]))
    for j0, n in rows:
        ptrs = [(out[f][j0:].data_ptr() if j0 < out[f].shape[0] else None) if f in out else None for f in sd.FIELDS]
        L.call("ogg_regional_stereo_band_dev", *(list(p) + [j0, n, ws.data_ptr(), wsb] + ptrs + [st]))
    return host(out)


@pytest.mark.parametrize("nx, delta", [(66, 0.125), (16, 4.0)])      # 4 degrees: the other form of the area's small arctangent (d > 1/16)
def test_every_split_into_bands(S, hip, nx, delta):
    """66 x 8 cells (and 16 x 8 coarse ones), 9 point rows: every split into one, two and three bands (1 + 8 + 28), in either order of the launches, the
    split into 9 bands of one row, and one band cut in the middle of the arrays give the whole grid's bytes; without metrics the same
    x and y bytes and nothing else."""
    args = dict(lon_c=-64.5, lat_c=89.7, nx=nx, ny=8, delta=delta, tilt=-17.0)     # the pole is inside a cell of the domain
    p = S.params(**args)
    assert len(S.poles(p)) == 1
    whole = run_bands(S, hip, p, [(0, 9)])
    assert all(np.all(np.isfinite(whole[f])) for f in sd.FIELDS)
    splits = [c for n in (1, 2) for c in itertools.combinations(range(1, 9), n)] + [tuple(range(1, 9))]
    assert len(splits) == 8 + 28 + 1
    for cuts in splits:
        edges = (0,) + cuts + (9,)
        rows = [(a, b - a) for a, b in zip(edges[:-1], edges[1:])]
        assert same_bytes(whole, run_bands(S, hip, p, rows)) == [], cuts
        assert same_bytes(whole, run_bands(S, hip, p, rows[::-1])) == [], cuts
    middle = run_bands(S, hip, p, [(3, 4)])       # rows 3 .. 6 alone: the same bytes there, nothing anywhere else
    for f in sd.FIELDS:
        assert middle[f][3:7].tobytes() == whole[f][3:7].tobytes(), f      # rows 3 .. 6 are cell rows too
        assert np.all(np.isnan(middle[f][:3])) and np.all(np.isnan(middle[f][7:])), f
    p0 = S.params(metrics=False, **args)
    for rows in ([(0, 9)], [(0, 4), (4, 5)], [(0, 1), (1, 7), (8, 1)]):
        xy = run_bands(S, hip, p0, rows, metrics=False)
        assert sorted(xy) == ["x", "y"] and same_bytes(whole, xy, ("x", "y")) == []


@pytest.mark.parametrize("nx, ny", SHAPES)
def test_the_three_entries_give_the_same_bytes(S, nx, ny):
    """the host-pointer entry (stereo_grid), the device entries in one band and in three (stereo_grid_dev), with and without metrics"""
    for lat_c, tilt in ((47.0, 25.0), (-90.0, -100.0)):
        args = dict(lon_c=179.9, lat_c=lat_c, nx=nx, ny=ny, delta=0.125, tilt=tilt)
        a = S.stereo_grid(**args)
        assert sorted(a) == sorted(sd.FIELDS) and all(a[f].shape == S.shapes(nx, ny)[f] for f in sd.FIELDS)
        assert same_bytes(a, host(S.stereo_grid_dev(**args))) == []
        assert same_bytes(a, host(S.stereo_grid_dev(bands=3, **args))) == []
        b = S.stereo_grid(metrics=False, **args)
        assert sorted(b) == ["x", "y"] and same_bytes(a, b, ("x", "y")) == []
        assert same_bytes(a, host(S.stereo_grid_dev(metrics=False, bands=2, **args)), ("x", "y")) == []
        ref = sd.stereo(Re=sd.RE, **args)
        for f in sd.FIELDS:       # not the truth test: a gross check that the shapes above hold the right grid
            assert sd.error(f, a[f], ref[f], 0.0).max() <= 1e-10, f


COMMAND = ["--lon_c", "-52.25", "--lat_c", "90", "--tilt", "33.0", "-r", "1", "--cells", "8", "8", "--no_changing_meta"]


def test_the_file_is_reproducible_and_its_attributes(S, tmp_path, capsys):
    """with --no_changing_meta the file is byte-identical between two runs, between one band and three, and through the forward of
    ``regional --kind stereographic``; --skip_metrics keeps the x and y bytes; the attributes state the kind, the rotation and the projection"""
    from ocean_model_grid_generator_amd import netcdf3
    from ocean_model_grid_generator_amd import regional as R
    files = {}
    for name, extra in (("a", []), ("b", []), ("three", ["--bands", "3"])):
        files[name] = str(tmp_path / (name + ".nc"))
        s = S.main(COMMAND + ["-f", files[name]] + extra)
    files["forwarded"] = str(tmp_path / "forwarded.nc")
    R.main(["--kind", "stereographic"] + COMMAND + ["-f", files["forwarded"]])
    printed = capsys.readouterr().out
    first = open(files["a"], "rb").read()
    assert all(open(files[n], "rb").read() == first for n in ("b", "three", "forwarded"))
    assert b"regional_projection" in first and b"history" not in first
    skipped = str(tmp_path / "skip.nc")
    S.main(COMMAND + ["-f", skipped, "--skip_metrics"])
    a, b = (netcdf3.read_doubles(f, names=("x", "y", "dx")) for f in (files["a"], skipped))
    assert same_bytes(a, b, ("x", "y")) == [] and np.all(b["dx"] == -1.0)
    g = netcdf3.read_doubles(files["a"], names=sd.FIELDS)
    assert g["x"].shape == (17, 17) and g["dx"].shape == (17, 16) and g["dy"].shape == (16, 17) and g["area"].shape == (16, 16)
    assert same_bytes(S.stereo_grid(-52.25, 90.0, 16, 16, 0.5, tilt=33.0), g) == []
    assert (g["x"][8, 8], g["y"][8, 8], g["angle_dx"][8, 8]) == (-52.25, 90.0, 33.0)
    atts = netcdf3.read_header(files["a"]).gatts
    assert atts["grid_kind"] == "regional stereographic" and "stereographic" in atts["regional_projection"]
    assert float(atts["regional_lon_c"][0]) == -52.25 and float(atts["regional_lat_c"][0]) == 90.0 and float(atts["regional_tilt"][0]) == 33.0
    assert float(atts["regional_delta"][0]) == 0.5 and float(atts["regional_Re"][0]) == sd.RE
    assert s["poles"] == {"north": {"point": [8, 8]}} and "the north pole is the supergrid point (j, i) = (8, 8)" in printed
    assert "stereographic grid of 16 x 16 supergrid cells" in printed and "closed form" in printed
    assert abs(s["area_relative_error"]) <= np.finfo(np.float64).eps * (16 * 16 + 16)      # a sum of nx ny rounded terms
    capsys.readouterr()


def plane_cell(lon, lat, lon_c, lat_c, tilt, delta, nx, ny):
    """the model cell (j, i) of a point by the inverse projection: its plane coordinates in supergrid steps, halved"""
    from regional_definition import rotation
    q = rotation(lat_c, tilt)
    lam, phi = np.radians(np.asarray(lon) - lon_c), np.radians(lat)
    p = np.stack([np.cos(phi) * np.cos(lam), np.cos(phi) * np.sin(lam), np.sin(phi)])
    c = [sum(q[k][m] * p[m] for m in range(3)) for k in range(3)]
    d = np.radians(delta)
    fi, fj = 2.0 * c[1] / (1.0 + c[0]) / d + nx // 2, 2.0 * c[2] / (1.0 + c[0]) / d + ny // 2
    return np.floor(0.5 * fj).astype(int), np.floor(0.5 * fi).astype(int)


@pytest.mark.parametrize("lat_c, lon_c, tilt", [(90.0, -52.25, 33.0), (-90.0, 100.0, 0.0)])
def test_round_trip_of_a_pole_holding_grid_through_the_analyses(S, tmp_path, capsys, lat_c, lon_c, tilt):
    """16 x 16 supergrid cells of 1/2 degree about a pole, written by the command and read back by the file-based analyses.  The pole is
    the common corner of four model cells, and the cut of x runs from it along the meridian opposite lon_c, between two columns or rows
    of cells or through them, depending on the tilt.
      grid_quality   every figure finite, no seam, aspect ratios and corners those of a conformal grid;
      topography     a global quarter-degree int16 raster of 100 x latitude: every cell gets samples and its mean is 100 x the latitude
                     of its centre within 100 x (1/8 degree, half a raster step, + 0.15 degrees, the mean latitude of a one-degree cell
                     at the pole against its centre's: 0.06 degrees at the pole cell);
      locate         every model cell's centre lands in its own cell, and points within 0.1 degrees of the pole on either side of the
                     cut, and farther along it, land in the cell the inverse projection gives."""
    from ocean_model_grid_generator_amd import grid_quality as GQ
    from ocean_model_grid_generator_amd import locate as LOC
    from ocean_model_grid_generator_amd import netcdf3
    from ocean_model_grid_generator_amd import topography as T
    path = str(tmp_path / "ocean_hgrid.nc")
    S.main(["--lon_c", str(lon_c), "--lat_c", str(lat_c), "--tilt", str(tilt), "-r", "1", "--cells", "8", "8", "--no_changing_meta", "-f", path])
    capsys.readouterr()
    g = netcdf3.read_doubles(path, names=sd.FIELDS)
    sgn = 1.0 if lat_c > 0 else -1.0
    # grid quality
    rep = GQ.check_file(path)
    q = rep["grid"]
    assert rep.get("joints", []) == []
    figures = [q["dx"]["min"]["value"], q["dx"]["max"]["value"], q["dy"]["min"]["value"], q["dy"]["max"]["value"], q["area"]["min"]["value"],
               q["aspect_ratio_max"]["value"], q["rx_max"]["value"], q["ry_max"]["value"], q["corner"]["delta_max_deg"]["value"]]
    with capsys.disabled():
        print("\nstereo round trip lat_c=%g: grid quality %s" % (lat_c, " ".join("%.6g" % v for v in figures)))
    assert np.all(np.isfinite(figures)) and q["dx"]["min"]["value"] == g["dx"].min() and q["dx"]["n_degenerate"] == 0
    assert q["aspect_ratio_max"]["value"] < 1.01 and q["corner"]["delta_max_deg"]["value"] < 0.1 and q["corner"]["n_degenerate"] == 0
    # topography
    lat_band = -90.0 + 0.25 * (np.arange(720) + 0.5)
    raster = np.repeat(np.round(100.0 * lat_band).astype(np.int16)[:, None], 1440, axis=1)
    res = T.topography(g["x"], g["y"], raster, lon0=-180.0, dlon=0.25, lat0=-90.0, dlat=0.25)
    centre = g["y"][1::2, 1::2]
    worst = np.abs(res["height"] - 100.0 * centre).max()
    with capsys.disabled():
        print("stereo round trip lat_c=%g: topography samples %d .. %d, empty cells %d, |mean - 100 lat| <= %.2f" % (
            lat_c, res["n_samples"].min(), res["n_samples"].max(), res["summary"]["n_empty_cells"], worst))
    assert res["height"].shape == (8, 8) and res["summary"]["n_empty_cells"] == 0 and np.all(res["n_samples"] > 0)
    assert worst <= 100.0 * (0.125 + 0.15)
    # locate
    cx, cy = g["x"][1::2, 1::2].reshape(-1), g["y"][1::2, 1::2].reshape(-1)
    cut = lon_c + 180.0
    near = [(cut - 1.0, sgn * 89.95), (cut + 1.0, sgn * 89.95), (cut - 0.5, sgn * 88.4), (cut + 0.5, sgn * 88.4), (lon_c + 10.0, sgn * 89.93),
            (lon_c + 100.0, sgn * 87.2)]
    lon = np.concatenate([cx, [a for a, _ in near]])
    lat = np.concatenate([cy, [b for _, b in near]])
    loc = LOC.locate(g["x"], g["y"], lon, lat)
    wj, wi = plane_cell(lon, lat, lon_c, lat_c, tilt, 0.5, 16, 16)
    assert np.array_equal(wj[:64] * 8 + wi[:64], np.arange(64))
    with capsys.disabled():
        print("stereo round trip lat_c=%g: locate cells %s, expected %s" % (lat_c, loc["cell"][64:].tolist(), (wj[64:] * 8 + wi[64:]).tolist()))
    assert np.array_equal(loc["cell"], wj * 8 + wi) and np.all(loc["margin"] > 0.0)
    assert not loc["periodic"] and not loc["fold"]
