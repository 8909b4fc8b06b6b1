"""WHOLE small caps against the 50-digit truth (tests/golden/truth_small_caps.npz, scripts/truth_table.py --groups small): every point of
the bipolar caps of the plans at inverse resolution 0.25 (Ni = 180, so the pole columns Ni/4 = 45 are odd) and 0.5, and of the kept rows of
two displaced-pole caps at 0.5 (--r_dp 0.2; --lat_dp -85.85 --lon_dp 80) -- x, y and angle_dx, from the fused pass and from the
function-level path, with the caps' columns mirrored and evaluated one by one.  tests/test_gpu_truth.py holds the same fields to the same
truth at full size on sample rows; here nothing is sampled, so a single wrong point -- a lane-63/64 neighbour, one image column, a strip
end -- fails.

Bounds, in units of the fp64 reference's own distance from the truth as measured when the fixture was made (K_REF = 1.5, the project's
rule): coordinates per class (regular points, the five columns around each symmetry meridian, the top row) with the floors of
test_gpu_truth.py; the angle at every point with a stencil, |HIP - truth| <= K_REF * c_ref * shape + 8 ulp(180), where shape = 1 / hypot(N, D)
of the oracle's fp64 mesh (tests/angle_bounds.py) and c_ref = max(oracle error / shape) over the cap.  The measured distances go to the
file OGG_SMALL_CAPS_REPORT names, if set (profiles/small_caps_truth.json is one such run; tabulated in DESIGN.md section 2).
"""
import json
import os

import numpy as np
import pytest

import angle_bounds
from oracle import ogg_oracle as orc
from test_gpu_truth import K_REF, SYMS, err

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")
REPORT = {}
FLOOR = {"bipolar": 1e-13, "dpole": 3e-14}        # degrees: the coordinates' noise floor where the reference is exact (test_gpu_truth.py)
CAPS = {"sbp180_": ("bipolar", dict(inverse_resolution=0.25, ensure_nj_even=True)),
        "sbp360_": ("bipolar", dict(inverse_resolution=0.5, ensure_nj_even=True)),
        "sdp_rdp_": ("dpole", dict(inverse_resolution=0.5, r_dp=0.2, ensure_nj_even=True)),
        "sdp_latdp_": ("dpole", dict(inverse_resolution=0.5, lat_dp=-85.85, lon_dp=80.0, ensure_nj_even=True))}


def _save():
    out = os.environ.get("OGG_SMALL_CAPS_REPORT")
    if out:
        with open(out, "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)


@pytest.fixture(scope="module")
def truth():
    return np.load(os.path.join(GOLD, "truth_small_caps.npz"))


@pytest.fixture(scope="module")
def ogg(hip):
    import ocean_model_grid_generator_amd.ocean_grid_generator as m
    return m


def _pass_fields(flags, sym):
    """test_gpu_truth._pass_fields -- the fused pass of a whole grid on one GPU -- on the ORACLE's Mercator axis: the bipolar cap's lower
    latitude is read off that axis (OGG:1030), and the truth was made for the oracle's value of it.  The device's own axis is within 2 ulp
    of it (5e-14 degrees is its bound, test_gpu_parity.test_mercator_axis), but 2 ulp of lat0 move the whole cap by 1e-13 degrees, as much
    as the distances measured here; with the axis handed in, the pass and the truth start from the same bits."""
    from ocean_model_grid_generator_amd import supergrid
    Ni = int(flags["inverse_resolution"] * 720)
    y0, y1 = orc.mercator_y_star(Ni, -66.85954725, 64.05895973, True, flags["ensure_nj_even"])
    plan = supergrid.SupergridPlan(cap_symmetry=sym, mercator_axis=(y0, orc.phi_mercator(Ni, np.arange(y0, y1 + 1))), **flags)
    g = supergrid.Supergrid(plan, rank=0, world=1, device="cuda:0", halo="recompute")
    g.step()
    out = g.bands_to_host()
    g.close()
    return plan, out


def _pairs(k, bits):
    """The fixture's integers (truth = k 2^-bits degrees) as (..., 2) hi / lo pairs: hi = fp64(k 2^-bits), lo = the rest, exactly."""
    hi = np.ldexp(k.astype(np.float64), -bits)
    rest = k - np.ldexp(hi, bits).astype(np.int64)
    return np.stack([hi, np.ldexp(rest.astype(np.float64), -bits)], axis=-1)


@pytest.mark.parametrize("sym", SYMS)
@pytest.mark.parametrize("tag", sorted(CAPS))
def test_whole_small_cap_vs_truth(ogg, truth, tag, sym):
    kind, flags = CAPS[tag]
    bits = int(truth["fix_bits"])
    t = {f: _pairs(truth[tag + f], bits) for f in ("x", "y", "angle")}
    nrow, ncol = truth[tag + "x"].shape
    par = truth[tag + "params"]
    plan, fields = _pass_fields(flags, sym)
    top, ill = np.zeros((nrow, ncol), bool), np.zeros((nrow, ncol), bool)
    paths = {}
    if kind == "bipolar":
        Ni, Nj, lat0, lon_bp, rp = int(par[0]), int(par[1]), float(par[2]), float(par[3]), float(par[4])
        bp = next(s for s in plan.subs if s.name == "BP")
        assert (plan.Ni, bp.Nj, bp.nj1) == (Ni, Nj, nrow) and ncol == Ni + 1
        assert abs(bp.lat0_bp - lat0) < 1e-12 and abs(bp.lon_bp - lon_bp) < 1e-12 and abs(bp.rp - rp) < 1e-12
        assert bp.lat0_bp == lat0                                        # ... and the same bits (see _pass_fields)
        paths["pass"] = tuple(fields["BP"][f] for f in ("x", "y", "angle_dx"))
        x, y, _, _ = ogg.generate_bipolar_cap_mesh(Ni, Nj, lat0, lon_bp, ensure_nj_even=False, symmetry=sym)
        paths["functions"] = (x, y, ogg.angle_x(x, y))
        ox, oy, _, _ = orc.generate_bipolar_cap_mesh(Ni, Nj, lat0, lon_bp, ensure_nj_even=False)
        top[-1, :] = True
        for c in (Ni // 4, 3 * Ni // 4):
            ill[:-1, c - 2:c + 3] = True
    else:
        nx, ny, lon0, lat0, lon_dp, r_dp, row0 = int(par[0]), int(par[1]), float(par[2]), float(par[3]), float(par[4]), float(par[5]), int(par[6])
        assert int(par[7]) == nrow and ncol == nx + 1
        sc = plan.subs[0]
        assert sc.kind == "dpole" and (plan.Ni, sc.Nj) == (nx, ny) and sc.row0 <= row0 and sc.row0 + sc.nj1 == row0 + nrow == ny + 1
        assert abs(sc.lat0 - lat0) < 1e-12 and abs(sc.lon_dp - lon_dp) < 1e-12 and abs(sc.r_dp - r_dp) < 1e-12 and plan.lon0 == lon0
        paths["pass"] = tuple(fields["SC"][f][row0 - sc.row0:] for f in ("x", "y", "angle_dx"))
        x, y, _, _ = ogg.generate_displaced_pole_grid(nx, ny, lon0, lat0, lon_dp, r_dp)
        x, y = np.ascontiguousarray(x[row0:]), np.ascontiguousarray(y[row0:])
        paths["functions"] = (x, y, ogg.angle_x(x, y))
        ox, oy, _, _ = orc.generate_displaced_pole_grid(nx, ny, lon0, lat0, lon_dp, r_dp)
        ox, oy = ox[row0:], oy[row0:]
    shp = angle_bounds.shape(ox, oy)                                     # of the ORACLE's fp64 mesh
    fin = np.isfinite(shp)
    assert int((~fin).sum()) <= (1 if kind == "bipolar" else 0)          # the cap's top row at Ni/2: N == D == 0
    c_ref = float(truth[tag + "angle_c_ref"])
    abound = K_REF * c_ref * np.where(fin, shp, 0.0) + 8.0 * angle_bounds.ULP_180
    classes = [(nm, m) for nm, m in (("regular", ~top & ~ill), ("ill_columns", ill), ("top_row", top)) if m.any()]
    rep, failures = {}, []
    for path, (hx, hy, ha) in paths.items():
        assert hx.shape == hy.shape == ha.shape == (nrow, ncol), (path, hx.shape)
        for fld, v in (("x", hx), ("y", hy)):
            e = err(v, t[fld])
            for nm, m in classes:
                eref = float(truth["%s%s_eref_%s" % (tag, fld, nm)])
                bound = K_REF * max(eref, FLOOR[kind])
                rep["%s/%s/%s" % (path, fld, nm)] = {"oracle_vs_truth_deg": eref, "hip_vs_truth_deg": float(e[m].max()), "bound_deg": bound, "n": int(m.sum())}
                print("%s%s %s %s: oracle %.3e HIP %.3e bound %.3e deg" % (tag, path, fld, nm, eref, e[m].max(), bound))
                if not e[m].max() <= bound:
                    j, i = np.unravel_index(np.where(m, e, -1.0).argmax(), e.shape)
                    failures.append((path, fld, nm, int(j), int(i), float(e[j, i]), bound))
        e = err(ha, t["angle"])
        e = np.minimum(e, np.abs(e - 360.0))
        ratio = np.where(fin, e / abound, 0.0)
        ratio = np.where(np.isnan(ratio), np.inf, ratio)
        j, i = np.unravel_index(ratio.argmax(), ratio.shape)
        rep["%s/angle" % path] = {"c_ref_deg": c_ref, "hip_c_deg": float(np.where(fin, e / np.where(fin, shp, 1.0), 0.0).max()),
                                  "worst_d_over_bound": float(ratio.max()), "worst_j_i": [int(j), int(i)], "n": int(fin.sum())}
        print("%s%s angle: c_ref %.3e HIP c %.3e worst d / bound %.3f at (%d, %d)" % (tag, path, c_ref, rep["%s/angle" % path]["hip_c_deg"], ratio.max(), j, i))
        if ratio.max() > 1.0:
            order = np.argsort(ratio, axis=None)[::-1][:5]
            failures.append((path, "angle", [(int(a), int(b), float(e[a, b]), float(abound[a, b])) for a, b in zip(*np.unravel_index(order, ratio.shape))
                                             if ratio[a, b] > 1.0]))
    REPORT["%s%s" % (tag.rstrip("_"), "" if sym else "_every_column")] = rep
    _save()
    assert not failures, failures
