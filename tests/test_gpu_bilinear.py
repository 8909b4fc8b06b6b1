"""GPU tests of the bilinear interpolation (csrc/ogg_bilinear.hip, bilinear.py, Supergrid.bilinear): values and flags bit for bit
against the definition in tests/bilinear_definition.py at the h, u and v points, vectors at the h and c points before and after the
rotation, the fill against remap_definition.fill, for the remap tests' grids and sources (float32 and fp64, with and without missing
values and a wet mask); the same bits for any knob, run, entry point and rank count; a uniform wind and the lat-lon rows of a grid
with both caps; main(), the function-level path and the file command writing the same bytes (a rotated vector: each path against the
file command on the grid file it wrote, because the two paths' angle_dx differ in the last bits on the bipolar cap)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bilinear_definition as D
from test_gpu_remap import CASES, device_grid, edges, field, wet_of, write_sources

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# The filled results of every grid are compared: on NUMPY_FILL_GRIDS with remap_definition.fill itself, on the other three with the remap's
# fill step (remap.fill_dev) applied to the DEFINITION's interpolated values and flags, with the topology found from the stitched host
# arrays.  tests/test_gpu_remap.py holds that fill step to remap_definition.fill bit for bit on all five grids, and the numpy fill
# takes minutes per case on the larger grids; what is new here -- bilinear_dev's own topology detection, the layout of the values and
# flags it hands to the fill, one copy of the flags per component -- is compared on every grid either way.
NUMPY_FILL_GRIDS = ("r1", "r2_dp")
KNOBS = (("OGG_BILINEAR_RECORDS", ("1", "2", "3")), ("OGG_BILINEAR_BLOCKS", ("1", "7", "100000")), ("OGG_BILINEAR_LDS", ("0",)))


@pytest.fixture(scope="module")
def sg(hip):
    import ocean_model_grid_generator_amd.supergrid as m
    return m


def sources(kind, dtype, missing, nrec):
    """a scalar and the two components of a vector on the remap tests' source; with ``missing`` the components miss different cells"""
    from ocean_model_grid_generator_amd import remap as R
    lon, lat = edges(kind)
    fills = (-999.0,) if missing else ()
    t = field(lon, lat, nrec, dtype, missing)
    u = field(lon, lat, nrec, dtype, missing)[::-1].copy() * dtype(0.5) - dtype(7.0)
    v = (field(lon, lat, nrec, dtype, False) * dtype(-0.25) + dtype(3.0)).astype(dtype)
    if missing:
        u[u == dtype(-999.0 * 0.5 - 7.0)] = dtype(-999.0)
        v[:, 60:75, 200:230] = np.nan
    return (lon, lat), [R.Source(a, lon, lat, fill=fills, name=n) for a, n in ((t, "t"), (u, "u"), (v, "v"))]


def same(a, b, what):
    assert a.shape == b.shape and a.tobytes() == b.tobytes(), what


def want_fill(v, fl, res, fill_max=None, ref=None):
    """the definition's interpolated values and flags, filled: by remap_definition.fill, or (ref = (source, periodic, fold) found from
    the host arrays) by the remap's fill step on the device; the result's own summary must name that topology"""
    s = res["summary"]
    if ref is None:
        v, fl, _ = D.fill(v, fl, s["periodic"], s["fold"], fill_max)
        return v, fl
    import torch
    from ocean_model_grid_generator_amd import _lib as L
    from ocean_model_grid_generator_amd import remap as R
    src, periodic, fold = ref
    assert (s["periodic"], s["fold"]) == (periodic, fold)
    dev = torch.device("cuda:0")
    rs = (src.nrec,) + v.shape[-2:]
    tv = torch.from_numpy(np.ascontiguousarray(v.reshape(rs))).to(dev)
    tf = R.flags_buffer(torch, tv.numel(), dev).view(rs)
    tf.copy_(torch.from_numpy(np.ascontiguousarray(fl.reshape(rs))))
    counts = torch.zeros(len(L.REMAP_COUNT_FIELDS), dtype=torch.int64, device=dev)
    R.fill_dev(R.params(rs[1], rs[2], src, 0, periodic, fold, fill_max), tv, tf, counts, torch.cuda.current_stream(dev).cuda_stream, dev)
    return tv.cpu().numpy().reshape(v.shape), tf.cpu().numpy().reshape(fl.shape)


def check_rot(res, angle, kind, sfx=""):
    ca, sa = D.rot(D.points(angle, kind))
    assert np.abs(res["rot_cos" + sfx] - ca).max() <= 4e-16 and np.abs(res["rot_sin" + sfx] - sa).max() <= 4e-16, (kind, sfx)


@pytest.mark.parametrize("name", ["r1", "r2", "r2_dp", "r2_nosc", "om4"])
def test_device_equals_definition(sg, name):
    plan, ranks = device_grid(sg, name)
    g = ranks[0]
    cut = g.south_cut()
    out = sg.stitch(plan, [g.bands_to_host()])
    x, y, angle = out["x"], out["y"], out["angle_dx"]
    pts = {k: (D.points(x, k), D.points(y, k)) for k in "huv"}
    from ocean_model_grid_generator_amd import ocean_mask as M
    topo = M.detect_topology(x, y, 2)
    assert topo == (True, True)   # every grid here is periodic and folded along its top row
    for kind, dtype, missing, masked, nrec in CASES:
        (lon, lat), (t, u, v) = sources(kind, dtype, missing, nrec)
        mask = wet_of(x, y) if masked else None
        tag = (name, kind, dtype.__name__, missing, masked)
        # scalars at the h (masked), u and v points; no point is left out
        for k in "huv":
            res = g.bilinear(cut, t, points=k, mask=mask if k == "h" else None, fill=False)
            wv, wf = D.interpolate(*pts[k], lon, lat, t.records, fills=t.fill, mask=mask if k == "h" else None)
            same(res["values"], wv, tag + (k, "values"))
            same(res["flags"], wf, tag + (k, "flags"))
            assert res["counts"]["interpolated"] > 0 and res["counts"]["dry"] == (nrec * int((mask == 0).sum()) if k == "h" and masked else 0)
            if k == "h":   # the fill: the remap's, on the interpolated values and flags
                ref = None if name in NUMPY_FILL_GRIDS else (t,) + topo
                fres = g.bilinear(cut, t, mask=mask)
                fv, ff = want_fill(wv, wf, fres, ref=ref)
                same(fres["values"], fv, tag + ("filled values",))
                same(fres["flags"], ff, tag + ("filled flags",))
                assert (fres["counts"]["filled"] > 0) == bool(missing)
        # vectors at the h points: before the rotation, after it, and filled before it
        (wu, wv), wf = D.interpolate(*pts["h"], lon, lat, u.records, v.records, fills=u.fill, mask=mask)
        res = g.bilinear(cut, u, v, mask=mask, fill=False, rotate=False)
        for key, want in (("values", wu), ("values2", wv), ("flags", wf), ("flags2", wf)):
            same(res[key], want, tag + ("vector h", key))
        check_rot(res, angle, "h")
        for fill in (False, True) if missing else (False,):
            res = g.bilinear(cut, u, v, mask=mask, fill=fill)
            check_rot(res, angle, "h")
            fu, ff = want_fill(wu, wf, res, ref=ref and (u,) + topo) if fill else (wu, wf)
            fv, ff2 = want_fill(wv, wf, res, ref=ref and (v,) + topo) if fill else (wv, wf)
            assert ff.tobytes() == ff2.tobytes()
            ug, vg = D.rotate(fu, fv, ff, res["rot_cos"], res["rot_sin"])
            for key, want in (("values", ug), ("values2", vg), ("flags", ff), ("flags2", ff)):
                same(res[key], want, tag + ("rotated h", fill, key))
            assert res["summary"]["grid_relative"] and (res["counts"]["filled"] > 0) == fill
        # vectors at the c points: the first component at u, the second at v
        (uu, vu), fu_ = D.interpolate(*pts["u"], lon, lat, u.records, v.records, fills=u.fill)
        (uv, vv), fv_ = D.interpolate(*pts["v"], lon, lat, u.records, v.records, fills=u.fill)
        res = g.bilinear(cut, u, v, points="c", rotate=False)
        for key, want in (("values", uu), ("values2", vv), ("flags", fu_), ("flags2", fv_)):
            same(res[key], want, tag + ("vector c", key))
        res = g.bilinear(cut, u, v, points="c")
        check_rot(res, angle, "u")
        check_rot(res, angle, "v", "2")
        ug, _ = D.rotate(uu, vu, fu_, res["rot_cos"], res["rot_sin"])
        _, vg = D.rotate(uv, vv, fv_, res["rot_cos2"], res["rot_sin2"])
        for key, want in (("values", ug), ("values2", vg), ("flags", fu_), ("flags2", fv_)):
            same(res[key], want, tag + ("rotated c", key))
        if missing:
            assert np.any(fu_ == D.UNFILLED) and np.all(res["values"][fu_ == D.UNFILLED] == D.FILL)


def test_fill_max_and_an_unreachable_wet_cell(hip):
    from ocean_model_grid_generator_amd import bilinear as B
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    from ocean_model_grid_generator_amd import remap as R
    out = ogg.main(1.0, gridfilename=None, ensure_nj_even=True, no_changing_meta=True, return_arrays=True)
    x, y = out["x"], out["y"]
    lon, lat = edges("regular")
    f = field(lon, lat, 1, np.float64, True)
    mask = wet_of(x, y)
    cy = y[1::2, 1::2]
    j = int(np.argmin(np.abs(cy[:, 0] - 30.0)))
    mask[j - 1:j + 2, 40:43] = 0
    mask[j, 41] = 1                          # one wet cell in a ring of land ...
    lc = 0.5 * (lon[1:] + lon[:-1])
    cxv = x[1::2, 1::2][j, 41] % 360
    f[0][:, np.abs(lc - cxv) < 3] = np.nan    # ... where the source has no value
    src = R.Source(f, lon, lat, fill=(-999.0,))
    res = B.bilinear(x, y, src, mask=mask)
    assert res["flags"][0, j, 41] == D.UNFILLED and res["values"][0, j, 41] == D.FILL
    wv, wf = D.interpolate(D.points(x, "h"), D.points(y, "h"), lon, lat, src.records, fills=src.fill, mask=mask)
    fv, ff = want_fill(wv, wf, res)
    same(res["values"], fv, "values")
    same(res["flags"], ff, "flags")
    assert res["counts"]["filled"] > 0 and res["summary"]["periodic"] and res["summary"]["fold"]
    lim = B.bilinear(x, y, src, mask=mask, fill_max=2)
    v2, f2 = want_fill(wv, wf, lim, fill_max=2)
    same(lim["values"], v2, "fill_max values")
    same(lim["flags"], f2, "fill_max flags")
    assert lim["counts"]["unfilled"] > res["counts"]["unfilled"]
    nof = B.bilinear(x, y, src, mask=mask, fill=False)
    same(nof["values"], wv, "no fill")
    assert nof["counts"]["filled"] == 0 and nof["counts"]["unfilled"] == res["counts"]["filled"] + res["counts"]["unfilled"]


KEYS = ("values", "flags", "values2", "flags2", "rot_cos", "rot_sin", "rot_cos2", "rot_sin2")


def same_result(a, b, what):
    assert sorted(k for k in KEYS if k in a) == sorted(k for k in KEYS if k in b), what
    for k in KEYS:
        if k in a:
            same(a[k], b[k], what + (k,))
    assert a["summary"] == b["summary"], what


def test_same_bits_for_every_knob_run_and_entry_point(sg, monkeypatch):
    from ocean_model_grid_generator_amd import bilinear as B
    plan, ranks = device_grid(sg, "r1")
    g = ranks[0]
    cut = g.south_cut()
    out = sg.stitch(plan, [g.bands_to_host()])
    x, y, angle = out["x"], out["y"], out["angle_dx"]
    _, (t, u, v) = sources("regular", np.float32, True, 5)
    mask = wet_of(x, y)
    runs = {"scalar h": lambda: g.bilinear(cut, t, mask=mask), "scalar v": lambda: g.bilinear(cut, t, points="v"),
            "vector h": lambda: g.bilinear(cut, u, v, mask=mask), "vector c": lambda: g.bilinear(cut, u, v, points="c")}
    want = {k: run() for k, run in runs.items()}
    for k, run in runs.items():
        same_result(run(), want[k], ("again", k))
    for knob, vals in KNOBS:
        for val in vals:
            monkeypatch.setenv(knob, val)
            for k, run in runs.items():
                same_result(run(), want[k], (knob, val, k))
            monkeypatch.delenv(knob)
    # the host-pointer entry on the stitched host arrays against the device path
    same_result(B.bilinear(x, y, t, mask=mask), want["scalar h"], ("host", "scalar h"))
    same_result(B.bilinear(x, y, t, points="v"), want["scalar v"], ("host", "scalar v"))
    same_result(B.bilinear(x, y, u, v, angle_dx=angle, mask=mask), want["vector h"], ("host", "vector h"))
    same_result(B.bilinear(x, y, u, v, angle_dx=angle, points="c"), want["vector c"], ("host", "vector c"))
    with pytest.raises(ValueError, match="OGG_BILINEAR_LDS"):
        monkeypatch.setenv("OGG_BILINEAR_LDS", "2")
        try:
            g.bilinear(cut, t)
        except Exception as e:   # the library's refusal, whatever exception class carries it
            raise ValueError(str(e))
    monkeypatch.delenv("OGG_BILINEAR_LDS")


def test_same_bits_for_any_rank_count(sg):
    _, (t, u, v) = sources("gaussian", np.float32, True, 2)
    want = None
    for world in (1, 2, 3):
        plan, ranks = device_grid(sg, "r2_dp", world)
        cut = ranks[0].south_cut()
        out = sg.stitch(plan, [g.bands_to_host() for g in ranks])
        mask = wet_of(out["x"], out["y"])
        got = {"vector h": ranks[0].bilinear(cut, u, v, mask=mask), "vector c": ranks[0].bilinear(cut, u, v, points="c"),
               "scalar u": ranks[0].bilinear(cut, t, points="u")}
        assert all(g.bilinear(cut, u, v, mask=mask) is None and g.bilinear(cut, t, points="u") is None for g in ranks[1:])
        if want is None:
            want = got
        for k in got:
            same_result(got[k], want[k], (world, k))


def test_skip_metrics_has_no_angle(sg):
    plan = sg.SupergridPlan(inverse_resolution=1.0, ensure_nj_even=True, skip_metrics=True)
    g = sg.Supergrid(plan, device="cuda:0")
    g.run_pass()
    cut = g.south_cut()
    _, (t, u, v) = sources("regular", np.float64, False, 1)
    with pytest.raises(ValueError, match="skip_metrics"):
        g.bilinear(cut, u, v)
    res = g.bilinear(cut, t)
    assert res["counts"]["interpolated"] == res["values"].size


def test_uniform_wind_and_the_lat_lon_rows(sg):
    """r2_dp has the bipolar cap and the displaced-pole cap, so angle_dx is not zero there.  A uniform eastward wind (1, 0) turns to
    (U rot_cos, -(U rot_sin)) bit for bit with U the interpolated first component, which the definition leaves within 8 roundings of
    1 (the weights of a point do not always add up to exactly 1); wherever U is exactly 1 that is (rot_cos, -rot_sin) bit for bit.  In
    the lat-lon rows, where angle_dx == 0, the rotated components equal the unrotated ones."""
    from ocean_model_grid_generator_amd import remap as R
    plan, ranks = device_grid(sg, "r2_dp")
    g = ranks[0]
    cut = g.south_cut()
    angle = D.points(sg.stitch(plan, [g.bands_to_host()])["angle_dx"], "h")
    lon, lat = edges("regular")
    one = R.Source(np.ones((1, 180, 360)), lon, lat, name="u")
    zero = R.Source(np.zeros((1, 180, 360)), lon, lat, name="v")
    raw = g.bilinear(cut, one, zero, rotate=False)
    res = g.bilinear(cut, one, zero)
    U = raw["values"][0]
    assert np.abs(U - 1.0).max() <= 8 * 2.0 ** -53 and np.all(raw["values2"] == 0.0)
    ca, sa = res["rot_cos"], res["rot_sin"]
    assert np.array_equal(res["values"][0], U * ca) and np.array_equal(res["values2"][0], -(U * sa))
    exact = U == 1.0
    print("uniform wind: U == 1 exactly at %.1f %% of the points" % (100 * exact.mean()))
    assert exact.mean() > 0.9
    same(res["values"][0][exact], ca[exact], "ug")
    same(res["values2"][0][exact] + 0.0, -sa[exact] + 0.0, "vg")   # (+ 0.0: -0.0 and +0.0 are the same component)
    assert np.abs(angle).max() > 10.0 and np.abs(sa).max() > 0.1
    # a real field in the lat-lon rows
    _, (t, u, v) = sources("gaussian", np.float64, True, 2)
    raw = g.bilinear(cut, u, v, rotate=False)
    res = g.bilinear(cut, u, v)
    rows = np.all(angle == 0.0, axis=1)
    assert rows.sum() > angle.shape[0] // 2 and not rows.all()
    for k in ("values", "values2", "flags"):
        assert np.array_equal(res[k][:, rows], raw[k][:, rows]), k
    assert not np.array_equal(res["values"][:, ~rows], raw["values"][:, ~rows])


def write_winds(tmp_path):
    """a 3-level float32 temperature with missing values and float64 winds (uwnd misses a box), on a 1-degree grid, NetCDF-3"""
    from ocean_model_grid_generator_amd import netcdf3
    lo, la = -180.0 + np.arange(360) + 0.5, -90.0 + np.arange(180) + 0.5
    L, A = np.meshgrid(lo, la)
    t = np.stack([28 * np.cos(np.radians(A)) - k * 3 + np.sin(np.radians(L)) for k in range(3)]).astype(np.float32)
    for k in range(3):
        t[k][((L > -5 + 3 * k) & (L < 65 - 3 * k) & (A > -35 + 2 * k) & (A < 55)) | (np.abs(A) > 78 - 4 * k)] = 1e20
    uw = 8.0 * np.cos(np.radians(A)) + np.sin(2 * np.radians(L))
    vw = 2.0 * np.sin(np.radians(3 * L)) * np.cos(np.radians(A))
    uw[(L > 150) & (L < 170) & (A > -10) & (A < 10)] = 1e20
    src = str(tmp_path / "atm.nc")
    ds = netcdf3.Dataset(src, [("depth", 3), ("lat", 180), ("lon", 360)])
    ds.def_var("depth", netcdf3.NC_DOUBLE, ("depth",), [("units", "m")], np.array([0.0, 100.0, 1000.0]))
    ds.def_var("lat", netcdf3.NC_DOUBLE, ("lat",), [("units", "degrees_north")], la)
    ds.def_var("lon", netcdf3.NC_DOUBLE, ("lon",), [("units", "degrees_east")], lo)
    ds.def_var("t_an", netcdf3.NC_FLOAT, ("depth", "lat", "lon"), [("units", "degC"), ("_FillValue", 1e20)], t)
    ds.def_var("uwnd", netcdf3.NC_DOUBLE, ("lat", "lon"), [("units", "m s-1"), ("_FillValue", 1e20)], uw)
    ds.def_var("vwnd", netcdf3.NC_DOUBLE, ("lat", "lon"), [("units", "m s-1"), ("_FillValue", 1e20)], vw)
    ds.write()
    return src


def test_main_function_level_and_file_command_write_the_same_bytes(hip, tmp_path, capsys):
    from ocean_model_grid_generator_amd import netcdf3
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    topo, _ = write_sources(tmp_path)
    src = write_winds(tmp_path)
    f = {k: str(tmp_path / (k + ".nc")) for k in ("grid", "grid2", "plain", "topog", "t2", "i1", "i2", "i3", "i4", "c1", "c2", "c3")}
    kw = dict(no_changing_meta=True, ensure_nj_even=True, topog_source=topo, interp_source=src, interp_var=["t_an"],
              interp_vector=[["uwnd", "vwnd"]])
    ogg.main(1.0, gridfilename=f["grid"], topog_file=f["topog"], interp_file=f["i1"], **kw)
    ogg.main(1.0, gridfilename=f["grid2"], topog_file=f["t2"], interp_file=f["i2"], path="functions", **kw)
    out = capsys.readouterr().out
    assert "bilinear: t_an, 3 records" in out and "bilinear: vector (uwnd, vwnd), grid-relative" in out
    cmd = [sys.executable, "-m", "ocean_model_grid_generator_amd.bilinear"]
    for grid, topog, o in ((f["grid"], f["topog"], f["i3"]), (f["grid2"], f["t2"], f["i4"])):
        r = subprocess.run(cmd + [grid, src, "--var", "t_an", "--vector", "uwnd", "vwnd", "--topog", topog, "-o", o], cwd=ROOT,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
    # each path's file is the file command's on the grid file that path wrote, byte for byte
    b1, b2 = open(f["i1"], "rb").read(), open(f["i2"], "rb").read()
    assert b1 == open(f["i3"], "rb").read() and b2 == open(f["i4"], "rb").read()
    # between the two paths the scalar and every flag are the same bytes; the rotated components are the same bytes wherever the
    # paths' angle_dx is: the function-level path takes the bipolar cap's angle from the stored mesh, the pass inside the mesh kernel
    # (tests/test_gpu_pipeline.py, _same_as_function_level: < 1e-10 degrees apart), so there they agree to that angle times the speed
    h = netcdf3.read_header(f["i1"])
    h2 = netcdf3.read_header(f["i2"])
    ang = [np.frombuffer(netcdf3.read_var_bytes(g, netcdf3.read_header(g), "angle_dx"), dtype=">f8") for g in (f["grid"], f["grid2"])]
    nxp = 2 * h.vars["uwnd"].shape[1] + 1
    same_angle = np.all((ang[0] == ang[1]).reshape(-1, nxp)[1::2, 1::2], axis=1)
    assert same_angle.sum() > same_angle.size // 2
    for name in ("t_an", "t_an_interp_flag", "uwnd_interp_flag", "vwnd_interp_flag", "uwnd", "vwnd"):
        dt = netcdf3.NC_BYTE if name.endswith("flag") else netcdf3.NC_DOUBLE
        a, b = (np.frombuffer(netcdf3.read_var_bytes(p, hh, name, dtype=dt), dtype=np.int8 if name.endswith("flag") else ">f8")
                for p, hh in ((f["i1"], h), (f["i2"], h2)))
        if name in ("uwnd", "vwnd"):
            a, b = a.reshape(h.vars[name].shape), b.reshape(h.vars[name].shape)
            assert a[same_angle].tobytes() == b[same_angle].tobytes(), name
            print("%s: pass path against function-level path, largest difference %.3e" % (name, np.abs(a - b).max()))
            assert np.abs(a - b).max() <= 10.0 * np.radians(1e-9), name
        else:
            assert a.tobytes() == b.tobytes(), name
    # the grid file does not change with the new flags
    ogg.main(1.0, gridfilename=f["plain"], no_changing_meta=True, ensure_nj_even=True)
    assert open(f["plain"], "rb").read() == open(f["grid"], "rb").read()
    assert h.vars["t_an"].shape[0] == 3 and "depth" in h.vars and h.vars["t_an_interp_flag"].nc_type == netcdf3.NC_BYTE
    assert h.vars["uwnd"].atts["grid_relative"] == "true" and h.vars["vwnd"].atts["vector_partner"] == "uwnd"
    flags = np.frombuffer(netcdf3.read_var_bytes(f["i1"], h, "t_an_interp_flag", dtype=netcdf3.NC_BYTE), dtype=np.int8)
    flags = flags.reshape(h.vars["t_an_interp_flag"].shape)
    depth = np.frombuffer(netcdf3.read_var_bytes(f["topog"], netcdf3.read_header(f["topog"]), "depth"), dtype=">f8")
    wet = (depth.reshape(flags.shape[1:]) > 0) & (depth.reshape(flags.shape[1:]) != 1e20)
    assert np.all(np.isin(flags[:, wet], (1, 2))) and np.all(flags[:, ~wet] == 0) and np.any(flags == 2)
    # the staggered points, unrotated, on the three paths too
    kw = dict(no_changing_meta=True, ensure_nj_even=True, interp_source=src, interp_vector=[["uwnd", "vwnd"]], interp_points="c",
              interp_no_rotate=True)
    ogg.main(1.0, gridfilename=None, interp_file=f["c1"], **kw)
    ogg.main(1.0, gridfilename=None, interp_file=f["c2"], path="functions", **kw)
    r = subprocess.run(cmd + [f["grid"], src, "--vector", "uwnd", "vwnd", "--points", "c", "--no_rotate", "-o", f["c3"]], cwd=ROOT, capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    c1 = open(f["c1"], "rb").read()
    assert c1 == open(f["c2"], "rb").read() and c1 == open(f["c3"], "rb").read()
    h = netcdf3.read_header(f["c1"])
    ny, nx = h.vars["uwnd"].shape[0], h.vars["vwnd"].shape[1]
    assert tuple(h.vars["uwnd"].shape) == (ny, nx + 1) and tuple(h.vars["vwnd"].shape) == (ny + 1, nx)
    assert h.vars["uwnd"].atts["grid_relative"] == "false"
    fl = np.frombuffer(netcdf3.read_var_bytes(f["c1"], h, "uwnd_interp_flag", dtype=netcdf3.NC_BYTE), dtype=np.int8)
    assert np.any(fl == 3) and np.all(np.isin(fl, (1, 3)))   # no fill at the staggered points: the box stays unfilled
