"""GPU tests of topography by refined sampling (csrc/ogg_topog.hip) on the hand-made grids and rasters of tests/small_grids.py:
every field of every record bit-identical to the numpy definition (tests/topog_definition.py), and, where the inputs are exact by
construction, to truths that do not come from the definition: closed forms in Python integers, mirrored grids, and grids or rasters
stated a whole turn away."""
import ctypes

import numpy as np
import pytest

import small_grids as G
import topog_definition as td
from test_gpu_topog import assert_records_equal

pytestmark = pytest.mark.gpu
SWEEP = (1, 2, 3, 7, 8, 31, 32, 33, 63, 64, 65, 96, 127, 128, 129, 255, 256)


@pytest.fixture(scope="module")
def T(hip):
    from ocean_model_grid_generator_amd import topography
    return topography


def source(T, kind):
    r = G.raster(kind)
    return T.Source(r["data"], *r["box"], fill=r["fill"], quantum=r["quantum"])


def definition(x, y, kind, **kw):
    r = G.raster(kind)
    kw.setdefault("cells_", "supergrid")
    return td.records(x, y, r["data"], *r["box"], quantum=r["quantum"], fill=r["fill"], **kw)


def check(T, x, y, kind, cells="supergrid", **kw):
    """the device's records of a grid against the definition's; returns them"""
    got = T.topography(x, y, source(T, kind), cells=cells, **kw)["records"]
    assert_records_equal(got, definition(x, y, kind, cells_=cells, **kw))
    return got


def same_records(a, b, what):
    for f in td.RECORD_FIELDS:
        np.testing.assert_array_equal(a[f], b[f], err_msg="%s: %s" % (what, f))


# ---- shapes, placements and cells ------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", G.RASTER_KINDS)
def test_every_shape_against_every_raster(T, kind):
    """1 x 1 cells, one row of 63, 64 and 65 cells (records that are no multiple of the four a wavefront takes at a time), one column
    of 129, an odd nx: supergrid cells always, model cells where both sizes are even, the refusal where they are not."""
    for name, (ny, nx, _) in G.TOPOG_SHAPES.items():
        x, y = G.shape_grid(name)
        check(T, x, y, kind)
        if ny % 2 == 0 and nx % 2 == 0:
            check(T, x, y, kind, cells="model")
        else:
            with pytest.raises(ValueError, match="model cells are 2 x 2 supergrid cells"):
                T.topography(x, y, source(T, kind), cells="model")


@pytest.mark.parametrize("kind", ["int16", "int16_fill2", "band60", "window", "window_m360", "float32_q0.01", "1x1_global", "ny1"])
def test_every_placement(T, kind):
    for name in G.PLACEMENTS:
        x, y = G.placed(name)
        check(T, x, y, kind)
        check(T, x, y, kind, cells="model")
    for sign in (1, -1):
        check(T, *G.beyond_pole_row(sign), kind)


@pytest.mark.parametrize("kind", ["int16", "band60", "window", "float64_q0.5"])
def test_pole_cells_and_odd_cells(T, kind):
    for name, (x, y, n_pole) in G.pole_cells().items():
        for refine in (None, 4):
            got = check(T, x, y, kind, refine=refine)
            assert int(got["n_pole"].sum()) == n_pole, name
    for name, (x, y) in G.odd_cells().items():
        for refine in (None, 5):
            check(T, x, y, kind, refine=refine)


def test_refine_sweep(T):
    """R below, at and above a wavefront's 64 lanes: the flattened sample walk with and without its carry"""
    x, y = G.shape_grid("2x2")
    for R in SWEEP:
        for kind in ("int16", "index_sum"):
            got = check(T, x, y, kind, refine=R)
            assert np.all(got["n"] + got["n_missing"] == R * R) and np.all(got["R"] == R)
        check(T, x, y, "int16_fill2", refine=R, cells="model")
    with pytest.raises(ValueError, match="refine must be"):
        T.topography(x, y, source(T, "int16"), refine=257)


# ---- values ----------------------------------------------------------------------------------------------------
def test_int16_fills(T, hip):
    L = hip
    x, y = G.placed("home")
    one, two = check(T, x, y, "int16_fill1"), check(T, x, y, "int16_fill2")
    assert one["n_missing"].sum() > 0 and two["n_missing"].sum() > one["n_missing"].sum()
    # a fill that no int16 equals (1e20, first or second) marks nothing; the other fill still does
    r = G.raster("int16_fill2")
    for fills, like in (((1.0e20, -32768.0), (-32768.0,)), ((32767.0, 1.0e20), (32767.0,)), ((1.0e20, 0.5), ())):
        src = T.Source(r["data"], *r["box"])       # the descriptor points into it
        desc = src.descriptor()
        desc.n_fill = 2
        desc.fill[0], desc.fill[1] = fills
        band = L.TopogBand(nx=x.shape[1] - 1, j0=0, n_cell_rows=x.shape[0] - 1, cells=L.TOPOG_SUPERGRID_CELLS, refine=0, oversample=2.0)
        band.x, band.y = L.ptr(x), L.ptr(y)
        rec = T.empty_records((x.shape[0] - 1, x.shape[1] - 1))
        L.call("ogg_topog", ctypes.byref(band), ctypes.byref(desc), rec.ctypes.data)
        assert_records_equal(rec, td.records(x, y, r["data"], *r["box"], fill=like, cells_="supergrid"))


@pytest.mark.parametrize("kind", G.FLOAT_RASTERS)
def test_float_rasters_ties_limits_and_refusals(T, kind):
    """values half-way between two steps, NaN and two fills; +-2^21 * quantum is accepted, one step more and an infinity are not"""
    x, y = G.placed("home")
    got = check(T, x, y, kind)
    assert got["n_missing"].sum() > 0 and got["n"].sum() > 0
    lim = check(T, *G.limit_grid(), kind)
    assert lim["max"][0, 0] == 2 ** 21 and lim["min"][1, 0] == -2 ** 21
    r = G.raster(kind)
    for bad in ((2 ** 21 + 1) * r["quantum"], -(2 ** 21 + 1) * r["quantum"], np.inf, -np.inf):
        d = r["data"].copy()
        d[G.LIMIT_ELEMENTS[1]] = bad
        src = T.Source(d, *r["box"], fill=r["fill"], quantum=r["quantum"])
        with pytest.raises(Exception, match="exceeds"):
            T.topography(x, y, src, cells="supergrid")
        with pytest.raises(ValueError, match="exceeds 2\\^21"):
            T.DeviceSource(src, "cuda:0")


@pytest.mark.parametrize("kind", ["int16", "float64_q0.01"])
def test_sea_level(T, kind):
    """n_wet against the definition's (double)q < wet_below for thresholds at, between and beyond the values"""
    x, y = G.placed("home")
    for level in (0.0, -0.5, 0.5, 1.0e30, -1.0e30, float("nan")):
        got = check(T, x, y, kind, sea_level=level)
        if level == 1.0e30:
            assert np.array_equal(got["n_wet"], got["n"])
        if level != level or level == -1.0e30:
            assert not got["n_wet"].any()


def test_capacity_of_the_integer_sums(T):
    """One model cell of 4 x 256 x 256 samples of q = +-2^21: the largest sums a record can hold, from Python integers."""
    x, y = G.shape_grid("2x2")
    for kind, sign in (("const_p", 1), ("const_m", -1)):
        rec = T.topography(x, y, source(T, kind), refine=256, cells="model")["records"]
        assert rec.shape == (1, 1)
        want = {"n": 2 ** 18, "n_missing": 0, "n_wet": 2 ** 18 if sign < 0 else 0, "sum": sign * 2 ** 39, "sumsq": 2 ** 60,
                "min": sign * 2 ** 21, "max": sign * 2 ** 21, "R": 256, "n_pole": 0, "n_clamped": 0}
        assert {f: int(rec[f][0, 0]) for f in want} == want


@pytest.mark.parametrize("kind", G.INDEX_RASTERS)
def test_index_rasters_closed_forms(T, kind):
    x, y = G.grid(6, 8)
    for R in (2, 8, 16, 64, 128):
        rec = T.topography(x, y, source(T, kind), refine=R, cells="supergrid")["records"]
        for j in range(6):
            for i in range(8):
                want = G.index_truth(kind, int(x[j, i] * 8), int(y[j, i] * 8), R)
                assert tuple(int(rec[f][j, i]) for f in ("n", "sum", "sumsq", "min", "max")) == want, (R, j, i)
    x, y = G.grid(1, 4, lon0=178.0)     # across the raster's seam
    rec = T.topography(x, y, source(T, kind), refine=8, cells="supergrid")["records"]
    for i in range(4):
        assert tuple(int(rec[f][0, i]) for f in ("n", "sum", "sumsq", "min", "max")) == G.index_truth(kind, int(x[0, i] * 8), int(y[0, i] * 8), 8)


@pytest.mark.parametrize("kind", ["int16", "window", "float64_q0.5", "index_sum"])
def test_mirrored_grids_give_mirrored_records(T, kind):
    x, y = G.placed("home")
    for refine in (8, 64):
        want = T.topography(x, y, source(T, kind), refine=refine, cells="supergrid")["records"]
        for sj, si in ((1, -1), (-1, 1), (-1, -1)):
            xm, ym = np.ascontiguousarray(x[::sj, ::si]), np.ascontiguousarray(y[::sj, ::si])
            got = T.topography(xm, ym, source(T, kind), refine=refine, cells="supergrid")["records"]
            same_records(got, want[::sj, ::si], "mirror %d %d" % (sj, si))


# ---- the two settled points ------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", G.REGIONAL_KINDS + ("int16", "int16_fill1", "band60", "1x1_global", "float32_q0.01", "float64_q0.5"))
def test_records_do_not_depend_on_the_longitude_branch(T, kind):
    """One property for every raster kind: x -> x + 360 k and lon0 -> lon0 +- 360 leave every record as it is.  A regional raster is
    met on its own branch: before that was settled, a grid or a window stated a turn away gave n = 0 in every cell, silently."""
    x, y = G.placed("home")
    r = G.raster(kind)
    want = check(T, x, y, kind)
    assert want["n"].sum() > 0
    for k in (-2, -1, 1, 10):
        same_records(check(T, x + 360.0 * k, y, kind), want, "k = %d" % k)
    for shift in (-360.0, 360.0):
        src = T.Source(r["data"], r["box"][0] + shift, *r["box"][1:], fill=r["fill"], quantum=r["quantum"])
        got = T.topography(x, y, src, cells="supergrid")["records"]
        same_records(got, want, "lon0 %+g" % shift)
    for name in ("m360", "p360", "m720", "p720", "p3600"):
        same_records(check(T, *G.placed(name), kind), want, name)


def test_the_window_stated_a_turn_away_is_the_same_raster(T):
    x, y = G.placed("home")
    want = check(T, x, y, "window")
    assert want["n"].sum() == 48 * 81 and not want["n_missing"].any()
    same_records(check(T, x, y, "int16"), want, "the big raster")
    for kind in ("window_p360", "window_m360"):
        same_records(check(T, x, y, kind), want, kind)
        same_records(check(T, x, y, kind, cells="model"), check(T, x, y, "window", cells="model"), kind)


@pytest.mark.parametrize("kind", ["int16", "band60", "window", "float64_q0.5"])
@pytest.mark.parametrize("coord", ["x", "y"])
@pytest.mark.parametrize("value", ["nan", "pinf", "minf"])
def test_a_point_that_is_not_finite_makes_its_cells_missing(T, kind, coord, value):
    """NaN, +inf and -inf in x and in y, at each of the four corner positions: the cell has n = 0, 65536 MISSING samples and a
    clamped R, for periodic and regional rasters alike; every other cell is as on the clean grid."""
    x, y, cells = G.nonfinite_grid(coord, value)
    got = check(T, x, y, kind)
    clean = check(T, *G.placed("home"), kind)
    hit = np.zeros(got.shape, dtype=bool)
    for j, i in cells:
        hit[j, i] = True
        assert (int(got["n"][j, i]), int(got["n_missing"][j, i]), int(got["n_clamped"][j, i]), int(got["R"][j, i])) == (0, 65536, 1, 256)
    assert got[~hit].tobytes() == clean[~hit].tobytes()
    model = check(T, x, y, kind, cells="model")
    assert int(model["n_clamped"].sum()) == 4
    check(T, x, y, kind, refine=8)     # with a given R nothing is clamped, and the cells are MISSING all the same


# ---- bands and device sources ----------------------------------------------------------------------------------
def band_records(T, L, x, y, desc, j0, n, cells, refine, pass_next):
    """ogg_topog on the supergrid rows j0 .. j0 + n - 1 alone: (first output row, records)"""
    nx = x.shape[1] - 1
    band = L.TopogBand(nx=nx, j0=j0, n_cell_rows=n, cells=cells, refine=refine, oversample=2.0)
    keep = [np.ascontiguousarray(a[j0:j0 + n + (0 if pass_next else 1)]) for a in (x, y)]
    band.x, band.y = L.ptr(keep[0]), L.ptr(keep[1])
    if pass_next:
        keep += [np.ascontiguousarray(x[j0 + n]), np.ascontiguousarray(y[j0 + n])]
        band.x_next, band.y_next = L.ptr(keep[2]), L.ptr(keep[3])
    sh = 1 if cells == L.TOPOG_MODEL_CELLS else 0
    rows = int(L.load().ogg_topog_band_out_rows(ctypes.byref(band)))
    assert rows == ((j0 + n - 1) >> sh) - (j0 >> sh) + 1
    rec = T.empty_records((rows, nx >> sh))
    L.call("ogg_topog", ctypes.byref(band), ctypes.byref(desc), rec.ctypes.data)
    return j0 >> sh, rec


@pytest.mark.parametrize("kind", ["int16_fill2", "window", "float32_q0.5"])
def test_every_split_into_bands(T, hip, kind):
    """Every split of the six rows into two and into three bands, with the next row given and left to follow in x: the merged
    records are the one-band records byte for byte (model cells: an odd j0 gives partial records that combine exactly)."""
    L = hip
    x, y = G.placed("home")
    src = source(T, kind)                          # the descriptor points into it
    desc = src.descriptor()
    splits = [(a,) for a in range(1, 6)] + [(a, b) for a in range(1, 6) for b in range(a + 1, 6)]
    for cells, name in ((L.TOPOG_MODEL_CELLS, "model"), (L.TOPOG_SUPERGRID_CELLS, "supergrid")):
        sh = 1 if name == "model" else 0
        one = T.topography(x, y, source(T, kind), cells=name)["records"]
        for k, cuts in enumerate(splits):
            edges = (0,) + cuts + (6,)
            pieces = [band_records(T, L, x, y, desc, a, b - a, cells, 0, pass_next=bool((k + n) % 2))
                      for n, (a, b) in enumerate(zip(edges[:-1], edges[1:]))]
            merged = T.assemble(pieces, 6 >> sh, 8 >> sh)
            assert merged.tobytes() == one.tobytes(), (name, cuts)


@pytest.mark.parametrize("kind", ["int16_fill2", "float32_q0.01", "float64_q0.5"])
def test_device_source_and_device_band(T, hip, kind):
    """one case per dtype through DeviceSource and band_records_dev: device pointers throughout"""
    import torch
    L = hip
    x, y = G.placed("across_180")
    dev = T.DeviceSource(source(T, kind), "cuda:0", sea_level=0.5)
    for cells, name in ((L.TOPOG_MODEL_CELLS, "model"), (L.TOPOG_SUPERGRID_CELLS, "supergrid")):
        xd, yd = torch.from_numpy(x).to("cuda:0"), torch.from_numpy(y).to("cuda:0")
        band = L.TopogBand(nx=8, j0=0, n_cell_rows=6, cells=cells, refine=0, oversample=2.0)
        band.x, band.y = xd.data_ptr(), yd.data_ptr()
        band.x_next, band.y_next = xd[6].data_ptr(), yd[6].data_ptr()
        m0, out, ws = T.band_records_dev(band, dev.desc, torch.cuda.current_stream().cuda_stream, xd.device)
        torch.cuda.synchronize()
        assert m0 == 0
        assert_records_equal(T.records_to_host(out), definition(x, y, kind, cells_=name, sea_level=0.5))
