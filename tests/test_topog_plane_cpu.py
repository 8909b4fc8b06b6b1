"""CPU tests of plane-fit topography: the numpy definition (tests/topog_plane_definition.py) and the host code of topography.py (the
exact centred moments, the fields, the merge of partial records, the file) on the hand-made grids and rasters of
tests/small_grids.py: rasters that ARE planes, planes added to a random raster, records that must not depend on how the raster or the
grid is stated or on the split into bands, every plane_flag on a named input, and the fp64 fields against exact rationals."""
from fractions import Fraction

import numpy as np
import pytest

import small_grids as G
import topog_definition as td
import topog_plane_definition as tp

from ocean_model_grid_generator_amd import _lib as L
from ocean_model_grid_generator_amd import netcdf3
from ocean_model_grid_generator_amd import topography as T


def as_struct(rec):
    out = T.empty_records(rec["n"].shape, plane=True)
    for f in tp.FIELDS:
        out[f] = rec[f]
    return out


def definition(x, y, kind, **kw):
    r = G.raster(kind)
    return tp.records(x, y, r["data"], *r["box"], quantum=r["quantum"], fill=r["fill"], **kw)


def host_fields(rec, y, cells, box, quantum=1.0):
    return T.fields_from_records(as_struct(rec), quantum, T.cell_latitudes(y, cells), box[1], box[3])


def same(a, b, what=""):
    for f in tp.FIELDS:
        np.testing.assert_array_equal(a[f], b[f], err_msg="%s: %s" % (what, f))


# ---- rasters that are planes -----------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,ab", [("index_is", (1.0, 0.0)), ("index_js", (0.0, 1.0)), ("index_sum", (1.0, 1.0))])
@pytest.mark.parametrize("cells", ["model", "supergrid"])
def test_index_rasters_are_planes(kind, ab, cells):
    """q = is, js, is + js: a = 1 or 0, b = 0 or 1 and h2 = 0 EXACTLY from the fp64 path, flag 1 on every cell.  (index_is is
    is mod 251 and the rasters jump at their seam, so the grids sit where the raster is one plane: the home placements.)"""
    for x, y in (G.placed("home"), G.shape_grid("5x3") if cells == "supergrid" else G.shape_grid("2x2"), G.placed("p360")):
        for refine in (None, 3):
            rec = definition(x, y, kind, cells_=cells, refine=refine)
            f = host_fields(rec, y, cells, G.GLOBAL_BOX)
            assert np.all(f["plane_flag"] == 1) and np.all(rec["n_far"] == 0)
            assert np.all(f["plane_a"] == ab[0]) and np.all(f["plane_b"] == ab[1]) and np.all(f["h2"] == 0.0)
            lat = T.cell_latitudes(y, cells)
            np.testing.assert_array_equal(f["slope_north"], ab[1] / (0.25 * np.pi / 180.0 * T.RE))
            np.testing.assert_array_equal(f["slope_east"], ab[0] / (0.25 * np.pi / 180.0 * T.RE * np.cos(lat * np.pi / 180.0)))


def seam_case():
    """a sheared 6 x 6 grid across the seam of a 360 x 720 raster (0.5 degree from -180) and the column count I' that runs on across it"""
    jj, ii = np.mgrid[0:7, 0:7]
    x, y = 176.25 + 1.25 * ii + 0.25 * jj, 38.125 + 1.125 * jj + 0.0625 * ii
    I, J = np.meshgrid(np.arange(720), np.arange(360))
    return np.ascontiguousarray(x), np.ascontiguousarray(y), (I + 360) % 720, J


def test_a_plane_across_the_raster_seam():
    """q = 3 I' - 7 J + 11 with I' continuous across the seam of the periodic raster: the periodic column offset follows it"""
    x, y, I, J = seam_case()
    raw = (3 * I - 7 * J + 11).astype(np.float64)
    for cells in ("model", "supergrid"):
        rec = tp.records(x, y, raw, -180.0, 0.5, -90.0, 0.5, quantum=1.0, cells_=cells)
        f = host_fields(rec, y, cells, (-180.0, 0.5, -90.0, 0.5))
        assert np.all(f["plane_flag"] == 1)
        assert np.all(f["plane_a"] == 3.0) and np.all(f["plane_b"] == -7.0) and np.all(f["h2"] == 0.0)


def test_an_added_plane_shifts_the_coefficients_and_leaves_h2():
    """random raster + (p I' + r J): the exact-rational a, b move by (p, r) and the exact-rational h2 does not move at all"""
    x, y, I, J = seam_case()
    base = np.random.default_rng(11).integers(-6000, 200, size=(360, 720))
    box = (-180.0, 0.5, -90.0, 0.5)
    for cells in ("model", "supergrid"):
        r0 = tp.records(x, y, base.astype(np.float64), *box, quantum=1.0, cells_=cells)
        for p, r in ((3, -7), (-40, 1), (0, 25)):
            r1 = tp.records(x, y, (base + p * I + r * J).astype(np.float64), *box, quantum=1.0, cells_=cells)
            for j in range(r0["n"].shape[0]):
                for i in range(r0["n"].shape[1]):
                    a0, b0, h0, _ = tp.rational_fit(tp.cell(r0, j, i))
                    a1, b1, h1, _ = tp.rational_fit(tp.cell(r1, j, i))
                    assert (a1 - a0, b1 - b0) == (p, r) and h1 == h0, (cells, p, r, j, i)


def test_the_moments_against_the_samples_themselves():
    """one model cell: the rational fit from the moments is the rational least-squares fit of its samples, listed one by one"""
    x, y = G.shape_grid("2x2", shear=True)
    r = G.raster("int16")
    rec = tp.records(x, y, r["data"], *r["box"], refine=5)
    c = td.cells(x, y, 0.25, 0.25, 5)
    flat = {k: v.reshape(-1) for k, v in c.items()}
    lon, lat = td.sample_positions(flat, 5, np.arange(4))
    q, _ = td.quantise(r["data"])
    v, miss = td.sample_values(q, *r["box"], lon, lat, flat["pole"])
    assert not miss.any()
    fi, fj = tp.sample_indices(1440, 720, *r["box"], lon, lat)
    a, b, h2, _ = tp.rational_fit(tp.cell(rec, 0, 0))
    want = tp.brute_fit([int(t) for t in fi.ravel()], [int(t) for t in fj.ravel()], [int(t) for t in v.ravel()])
    assert (a, b, h2) == want


# ---- records that do not depend on how things are stated -------------------------------------------------------
@pytest.mark.parametrize("cells", ["model", "supergrid"])
def test_records_do_not_depend_on_roll_turn_or_split(cells):
    x, y = G.placed("across_180")
    r = G.raster("int16_fill2")
    kw = dict(fill=r["fill"], cells_=cells)
    want = tp.records(x, y, r["data"], *r["box"], **kw)
    assert want["n"].sum() > 0 and want["n_missing"].sum() > 0 and not want["n_far"].any()
    # the raster rolled by k columns, lon0 moved by k * dlon
    for k in (1, 37, -700):
        got = tp.records(x, y, np.roll(r["data"], k, axis=1), r["box"][0] - k * r["box"][1], *r["box"][1:], **kw)
        same(got, want, "roll %d" % k)
    # the grid, or the raster's box, stated whole turns away (periodic and regional)
    for kind, place in (("int16_fill2", "home"), ("window", "across_window_lon0"), ("window", "home")):
        rr = G.raster(kind)
        xh, yh = G.placed(place)
        base = tp.records(xh, yh, rr["data"], *rr["box"], fill=rr["fill"], cells_=cells)
        for turn in (-720.0, -360.0, 360.0, 3600.0):
            same(tp.records(xh + turn, yh, rr["data"], *rr["box"], fill=rr["fill"], cells_=cells), base, "%s grid %+g" % (kind, turn))
        for turn in (-360.0, 360.0):
            same(tp.records(xh, yh, rr["data"], rr["box"][0] + turn, *rr["box"][1:], fill=rr["fill"], cells_=cells), base,
                 "%s lon0 %+g" % (kind, turn))
    # the rows split at every position (odd ones: two partial records of one model row, on one origin) and the pieces added
    sh = 1 if cells == "model" else 0
    whole = as_struct(want)
    for cuts in [(a,) for a in range(1, 6)] + [(1, 2), (1, 4), (3, 5), (2, 3)]:
        edges = (0,) + cuts + (6,)
        pieces = [(a >> sh, as_struct(tp.records(x[a:b + 1], y[a:b + 1], r["data"], *r["box"], j0=a, **kw)))
                  for a, b in zip(edges[:-1], edges[1:])]
        assert T.assemble(pieces[::-1], 6 >> sh, 8 >> sh).tobytes() == whole.tobytes(), cuts


def test_a_wrong_origin_would_show_in_the_split():
    """what the origin rule is for: partial records taken about each band's OWN first point row do not add up to the whole"""
    x, y = G.placed("home")
    r = G.raster("int16")
    whole = tp.records(x, y, r["data"], *r["box"])
    lower = tp.records(x[0:2], y[0:2], r["data"], *r["box"], j0=0)
    upper = tp.records(x[1:7], y[1:7], r["data"], *r["box"], j0=1)
    got = tp.add_records({f: v[:1] for f, v in upper.items()}, lower)
    same(got, {f: v[:1] for f, v in whole.items()}, "row 0 of two bands")
    wrong = tp.records(x[0:2], y[0:2], r["data"], *r["box"], cells_="supergrid")     # origins: each cell's own P00, a row below
    assert not np.array_equal(wrong["sy"][0, 0::2] + wrong["sy"][0, 1::2] + upper["sy"][0], whole["sy"][0])


# ---- flags -----------------------------------------------------------------------------------------------------
def flags_of(x, y, kind, cells, **kw):
    r = G.raster(kind)
    rec = definition(x, y, kind, cells_=cells, **kw)
    f = host_fields(rec, y, cells, r["box"], r["quantum"] or 1.0)
    d = tp.fields(rec, r["quantum"] or 1.0, tp.cell_latitudes(y, cells), r["box"][1], r["box"][3])
    for k in d:
        np.testing.assert_array_equal(f[k], d[k], err_msg=k)
    return rec, f


def pole_centre_without_longitude():
    """2 x 2 supergrid cells (one model cell) whose centre point is the north pole, its longitude NaN: three of the cells take their
    row neighbour's longitude for that corner and have samples, but the model cell has no origin"""
    x, y = G.grid(2, 2, lon0=30.0, lat0=88.0, d=1.0)
    y[1, 1], x[1, 1] = 90.0, np.nan
    return x, y


def test_every_flag_on_a_named_input():
    # 0: only missing samples (the rows of the grid above the window's top)
    rec, f = flags_of(*G.placed("above_window"), "window", "supergrid")
    assert np.all(f["plane_flag"][4:] == 0) and np.all(rec["n"][4:] == 0) and np.all(f["plane_flag"][:2] == 1)
    for k in ("h2", "plane_a", "plane_b", "slope_east", "slope_north"):
        assert np.all(f[k][4:] == T.FILL)
    # 2: one raster column (nx1) or one raster row (ny1): h2 is the variance about the mean
    for kind in ("nx1", "ny1"):
        for cells in ("model", "supergrid"):
            rec, f = flags_of(*G.placed("home"), kind, cells)
            hit = rec["n"] > 0
            assert hit.any() and np.all(f["plane_flag"][hit] == 2) and np.all(f["plane_flag"][~hit] == 0)
            var = T.exact_variance_numerator(rec["n"], rec["sum"], rec["sumsq"])[hit] / rec["n"][hit].astype(float) ** 2
            np.testing.assert_array_equal(f["h2"][hit], var)
            assert np.all(f["plane_a"][hit] == T.FILL) and np.all(f["slope_north"][hit] == T.FILL)
    # 3: a pole-enclosing cell: every valid sample of it is far
    for name, (x, y, n_pole) in G.pole_cells().items():
        rec, f = flags_of(x, y, "int16", "supergrid", refine=4)
        pole = rec["n_pole"] > 0
        assert int(pole.sum()) == n_pole
        assert np.all(f["plane_flag"][pole] == 3) and np.all(rec["n_far"][pole] == rec["n"][pole]) and not rec["n_far"][~pole].any()
        assert not np.any(f["plane_flag"][~pole] == 3), name
        if x.shape == (3, 3):    # the model cell of the block: refused through its one pole-enclosing cell
            rec, f = flags_of(x, y, "int16", "model", refine=4)
            assert f["plane_flag"][0, 0] == 3 and 0 < rec["n_far"][0, 0] < rec["n"][0, 0]
    # 3: no origin.  A point of nonfinite_grid that is not finite is a corner of every cell whose origin it is, so those cells have no
    # valid sample either (flag 0, n_far = 0) ...
    for coord in ("x", "y"):
        x, y, cells = G.nonfinite_grid(coord, "nan")
        rec, f = flags_of(x, y, "int16", "supergrid")
        j, i = G.NONFINITE_POINT
        assert f["plane_flag"][j, i] == 0 and rec["n_far"][j, i] == 0 and not rec["n_far"].any()
    # ... but a pole corner needs no longitude: a model cell centred on the pole, the pole's longitude NaN
    x, y = pole_centre_without_longitude()
    rec, f = flags_of(x, y, "int16", "model", refine=4)
    assert rec["n"][0, 0] == 3 * 16 and rec["n_far"][0, 0] == rec["n"][0, 0] and f["plane_flag"][0, 0] == 3
    assert f["h2"][0, 0] != T.FILL and f["plane_a"][0, 0] == T.FILL


def test_a_cell_half_a_turn_wide_is_far_on_a_fine_raster():
    """The offset rule alone, no raster allocated: a supergrid cell nearly half a turn wide (origin: its P00) against a periodic
    raster of Nx = 2^17 columns, Nx / 2 > 2^15: the samples beyond 2^15 columns from the origin are far, the others are not.  (170
    degrees wide: odd_cells()' cell of exactly 180 degrees counts as pole-enclosing by the winding rule, and is far for that.)"""
    assert td.cells(*G.odd_cells()["wide_180"], 0.25, 0.25)["pole"][0, 0] != 0
    x, y = G._cell((0.0, 170.0, 170.0, 0.0), (10.0, 10.0, 12.0, 12.0))
    Nx, Ny = 1 << 17, 1 << 16
    box = (-180.0, 360.0 / Nx, -90.0, 180.0 / Ny)
    c = td.cells(x, y, box[1], box[3], 64)
    flat = {k: v.reshape(-1) for k, v in c.items()}
    lon, lat = td.sample_positions(flat, 64, np.arange(1))
    fi, fj = tp.sample_indices(Nx, Ny, *box, lon, lat)
    fI0, fJ0, has = tp.origin_indices(*tp.origin_points(x, y, "supergrid"), Nx, Ny, *box)
    assert has.all()
    dI, dJ, near = tp.offsets(fi, fj, fI0[0, 0], fJ0[0, 0], has[0, 0], flat["pole"][:, None, None], Nx, True)
    assert dI.max() > tp.MAX_OFFSET and 0 < near.sum() < near.size
    np.testing.assert_array_equal(near, (np.abs(dI) <= tp.MAX_OFFSET) & (np.abs(dJ) <= tp.MAX_OFFSET))
    # the same cell against the 0.25-degree raster: nothing is far
    fi, fj = tp.sample_indices(1440, 720, *G.GLOBAL_BOX, lon, lat)
    fI0, fJ0, has = tp.origin_indices(*tp.origin_points(x, y, "supergrid"), 1440, 720, *G.GLOBAL_BOX)
    assert tp.offsets(fi, fj, fI0[0, 0], fJ0[0, 0], has[0, 0], 0, 1440, True)[2].all()
    # a regional raster does not wrap: a cell whose origin lies west of its branch cut at lon0 has an origin column of nearly a turn.
    # On the 0.25-degree window that is 1436 columns: every offset is shifted by it, within the limit, and the fit does not care ...
    xr, yr = G.grid(1, 1, lon0=99.0, lat0=0.0, d=2.0)
    rec = definition(xr, yr, "window", cells_="supergrid")
    n = int(rec["n"][0, 0])
    assert n > 0 and rec["n_missing"][0, 0] > 0 and rec["n_far"][0, 0] == 0 and -1436 * n <= rec["sx"][0, 0] <= -1433 * n
    inside = definition(xr + 1.0, yr, "window", cells_="supergrid", refine=int(rec["R"][0, 0]) * 2)    # 100 .. 102, origin inside
    assert tp.rational_fit(tp.cell(rec, 0, 0))[:2] != tp.rational_fit(tp.cell(inside, 0, 0))[:2]       # (other samples)
    # ... on a raster of 0.001 degree it is 359000 columns, and every sample is far
    fI0, fJ0, has = tp.origin_indices(xr[0, 0], yr[0, 0], 50000, 30000, 100.0, 0.001, -10.0, 0.001)
    lon, lat = np.array([100.0005, 100.5, 100.9995]), np.array([0.5, 1.0, 1.5])
    fi, fj = tp.sample_indices(50000, 30000, 100.0, 0.001, -10.0, 0.001, lon, lat)
    dI, dJ, near = tp.offsets(fi, fj, fI0, fJ0, has, 0, 50000, False)
    assert has and fI0 == 359000.0 and not near.any() and np.all(np.abs(dJ) <= tp.MAX_OFFSET)


# ---- the fp64 fields against the rational truth ----------------------------------------------------------------
H2_BOUND = 10 * 2.33e-16     # of Cqq / n^2
AB_BOUND = 10 * 1.03e-16     # of |a| + |b|


def test_fp64_fields_against_exact_rationals(capsys):
    """h2, a and b of topography.fields_from_records (centred moments rounded once, then the header's fp64 sequence) against the
    exact-rational solution of the same integer records, on the random 0.25-degree raster (with and without fill values, R from the
    spans and R = 9), a float raster quantised at 0.01, the window, and a raster that is a steep plane plus noise of a few quanta
    (the worst conditioning here: h2 is 1e-6 of the variance about the mean).  Measured worst errors on these inputs, over 1165 fitted
    cells: h2 2.33e-16 of Cqq / n^2, coefficients 1.03e-16 of |a| + |b|.  Asserted: ten times those."""
    worst_h2 = worst_ab = 0.0
    count = 0
    x, y, I, J = seam_case()
    steep = (40 * I - 25 * J + np.random.default_rng(5).integers(-3, 4, size=I.shape)).astype(np.float64)
    cases = [(G.placed(p), G.raster(k), kw) for p in ("home", "across_180", "above_band60") for k in ("int16", "int16_fill2", "band60")
             for kw in ({}, {"refine": 9})]
    cases += [(G.placed("home"), G.raster("float32_q0.01"), {}), (G.placed("across_window_lon0"), G.raster("window"), {}),
              ((x, y), dict(data=steep, box=(-180.0, 0.5, -90.0, 0.5), fill=(), quantum=1.0), {})]
    for (gx, gy), r, kw in cases:
        for cells in ("model", "supergrid"):
            rec = tp.records(gx, gy, r["data"], *r["box"], quantum=r["quantum"], fill=r["fill"], cells_=cells, **kw)
            quantum = td.quantise(r["data"], r["quantum"], r["fill"])[1]
            f = host_fields(rec, gy, cells, r["box"], quantum)
            q2 = Fraction(quantum) ** 2
            for j, i in zip(*np.nonzero(f["plane_flag"] == 1)):
                a, b, h2, var = tp.rational_fit(tp.cell(rec, j, i))
                if var == 0:
                    assert f["h2"][j, i] == 0.0
                    continue
                count += 1
                worst_h2 = max(worst_h2, float(abs(Fraction(f["h2"][j, i]) - h2 * q2) / (var * q2)))
                if a or b:
                    worst_ab = max(worst_ab, float((abs(Fraction(f["plane_a"][j, i]) - a) + abs(Fraction(f["plane_b"][j, i]) - b))
                                                   / (abs(a) + abs(b))))
    with capsys.disabled():
        print("\nplane fit, fp64 against rationals over %d cells: h2 %.3g of the variance, coefficients %.3g of |a| + |b|"
              % (count, worst_h2, worst_ab))
    assert count > 500
    assert worst_h2 <= H2_BOUND and worst_ab <= AB_BOUND


def test_exact_centred_moment_against_python_integers():
    rng = np.random.default_rng(9)
    n = rng.integers(1, 2 ** 18 + 1, size=3000)
    sa, sb = rng.integers(-2 ** 33, 2 ** 33, size=3000), rng.integers(-2 ** 39, 2 ** 39, size=3000)
    sab = rng.integers(-2 ** 54, 2 ** 54, size=3000)
    sab[::3] //= 2 ** 30                      # products below 2^64 as well as above
    sa[::5], sb[::7] = 0, 0
    got = T.exact_centred_moment(n, sab, sa, sb)
    want = np.array([float(int(a) * int(b) - int(c) * int(d)) for a, b, c, d in zip(n, sab, sa, sb)])
    np.testing.assert_array_equal(got, want)
    big = np.array([abs(int(a) * int(b) - int(c) * int(d)) >= 2 ** 64 for a, b, c, d in zip(n, sab, sa, sb)])
    assert big.any() and not big.all() and (want < 0).any() and (want > 0).any()
    lim = 2 ** 63 - 1
    for args in ((2 ** 18, 2 ** 54, 2 ** 33, 2 ** 39), (1, -lim, lim, lim), (lim, lim, -lim - 1, lim), (5, 0, 0, 7), (3, 12, 6, 6)):
        assert float(T.exact_centred_moment(*args)[0]) == float(args[0] * args[1] - args[2] * args[3]), args


# ---- interfaces ------------------------------------------------------------------------------------------------
def test_record_layout_constants_and_the_flag_that_needs_a_source():
    assert L.TOPOG_PLANE_RECORD.itemsize == 120 and L.load().ogg_abi_sizeof(L.ABI["TOPOG_PLANE_RECORD"]) == 120
    assert L.TOPOG_PLANE_RECORD.names[:len(L.TOPOG_RECORD.names)] == L.TOPOG_RECORD.names
    assert all(L.TOPOG_PLANE_RECORD.fields[f][1] == L.TOPOG_RECORD.fields[f][1] for f in L.TOPOG_RECORD.names)
    assert L.TOPOG_PLANE_RECORD.names[len(L.TOPOG_RECORD.names):] == tp.MOMENTS and L.TOPOG_PLANE_MAX_OFFSET == tp.MAX_OFFSET == 2 ** 15
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    assert ogg.AnalysisFlags().topog_roughness is False
    for path in ("pass", "functions"):
        with pytest.raises(ValueError, match="--topog_roughness needs --topog_source"):
            ogg.main(2.0, gridfilename=None, topog_roughness=True, path=path)
    args = ogg.build_parser().parse_args(["-r", "2", "--topog_source", "s.nc", "--topog_roughness"])
    assert args.topog_roughness is True and ogg.build_parser().parse_args(["-r", "2"]).topog_roughness is False
    with pytest.raises(ValueError, match="do not combine"):
        T.merge_into(T.empty_records((1, 1), plane=True), T.empty_records((1, 1)))
    with pytest.raises(ValueError, match="latitudes"):
        T.fields_from_records(T.empty_records((1, 1), plane=True), 1.0)


def test_topog_file_has_the_plane_variables_only_when_asked(tmp_path):
    x, y = G.placed("home")
    r = G.raster("int16")
    src = T.Source(r["data"], *r["box"])
    rec = as_struct(definition(x, y, "int16"))
    res = T.result(rec, 1.0, 0.0, "model", None, 2.0, src, T.cell_latitudes(y, "model"))
    assert res["summary"]["plane_flag_cells"] == [0, 12, 0, 0] and res["summary"]["n_far_samples"] == 0
    lines = T.summary_lines(res)
    assert "12 cells fitted, 0 degenerate, 0 refused" in lines[-2] and "largest h2" in lines[-1]
    p, p0 = str(tmp_path / "t.nc"), str(tmp_path / "t0.nc")
    T.write_topog(p, res)
    h = netcdf3.read_header(p)
    assert list(h.vars)[-4:] == ["h2", "slope_east", "slope_north", "plane_flag"]
    assert h.vars["h2"].atts["units"] == "m2" and h.vars["slope_east"].atts["units"] == "1" and h.vars["plane_flag"].nc_type == netcdf3.NC_BYTE
    for name in ("h2", "slope_east", "slope_north"):
        got = np.frombuffer(netcdf3.read_var_bytes(p, h, name), dtype=">f8").reshape(3, 4)
        np.testing.assert_array_equal(got, res[name])
    base = T.empty_records(rec.shape)
    for f in td.RECORD_FIELDS:
        base[f] = rec[f]
    res0 = T.result(base, 1.0, 0.0, "model", None, 2.0, src)
    T.write_topog(p0, res0)
    assert "h2" not in res0 and "plane_flag_cells" not in res0["summary"] and "h2" not in netcdf3.read_header(p0).vars
    for k in res0:
        if k not in ("records", "summary"):
            np.testing.assert_array_equal(res0[k], res[k])
    # the ocean mask's edit passes the new fields on
    from ocean_model_grid_generator_amd import ocean_mask as M
    edited = M.edit_topog(res, {"depth": res["depth"] * 2})
    assert all(edited[k] is res[k] for k in ("h2", "slope_east", "slope_north", "plane_a", "plane_b", "plane_flag"))
    T.write_topog(p0, edited)
    assert list(netcdf3.read_header(p0).vars)[-5:] == ["h2", "slope_east", "slope_north", "plane_flag", "depth_sampled"]
