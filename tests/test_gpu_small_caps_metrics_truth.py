"""EVERY dx, dy and area of four WHOLE small caps against the 50-digit truth (tests/golden/truth_small_caps_metrics*.npz, scripts/truth_table.py
--groups small_metrics; the caps of tests/test_gpu_small_caps_truth.py): the bipolar quadrature of order 5 with the top edge row of dx and
the last column of dy, the displaced-pole quadrature of order 4 on the rows main() keeps (truths A and B) -- from the fused PASS (what
main() and bench.py run; until now held to the oracle by test_gpu_parity.SUB_TOL only, 7e-10 relative on these displaced-pole caps) and from
the function-level entry points, with the caps' columns mirrored and evaluated one by one, the bipolar guard at its default and with every
cell literal (OGG_BP_GUARD_K=0), both arc forms of the displaced pole -- and the other coded orders (2, 3, 4 / 2) on reduced row sets.
tests/test_gpu_truth.py holds the same kernels to the same truth at full size on sampled cells; here nothing is sampled, so one wrong
cell -- a lane-63/64 neighbour, one image column, a strip end, one cell of the guard's fix-up list -- fails.

Every element is held to K_REF * max(the oracle's own distance from the truth in its class, floor) by tests/quad_bounds.py (classes from
the reference's conditioning only; planted defects: tests/test_quad_bounds_cpu.py).  Mirror-image elements are reported as lines of their
own ("<class>@image") under the bound of their class.  The measured distances go to the file OGG_SMALL_CAPS_METRICS_REPORT names, if set
(profiles/small_caps_metrics_truth.json is one such run; tabulated in DESIGN.md section 2).
"""
import json
import os

import numpy as np
import pytest

import quad_bounds as qb
from test_gpu_small_caps_truth import CAPS, _pass_fields
from test_gpu_truth import SYMS

pytestmark = pytest.mark.gpu

REPORT = {}
BIPOLAR = [t for t in sorted(CAPS) if CAPS[t][0] == "bipolar"]
DPOLE = [t for t in sorted(CAPS) if CAPS[t][0] == "dpole"]


@pytest.fixture(scope="module")
def ogg(hip):
    import ocean_model_grid_generator_amd.ocean_grid_generator as m
    return m


def _held(case, arrays, tag, order=None, image=None):
    """quad_bounds.check, with the measured distances recorded whether it passes or not."""
    rep = {}
    try:
        rep = qb.check(*arrays, tag, order=order, image=image, name=case)
    except qb.QuadBoundError as e:
        rep = dict(e.rep, failed=str(e))
        raise
    finally:
        REPORT[case] = rep
        for key, r in sorted(rep.items()):
            if key != "failed":
                print("%s %s: oracle %.3e HIP %.3e bound %.3e (%d)" % (case, key, r["oracle_vs_truth"], r["vs_truth"], r["bound"], r["n"]))
        out = os.environ.get("OGG_SMALL_CAPS_METRICS_REPORT")
        if out:
            with open(out, "w") as f:
                json.dump(REPORT, f, indent=1, sort_keys=True)
    return rep


def _bipolar_image(s, mirrored):
    """The elements whose value is a mirror image: the rows below the guard, the columns outside the three runs of QuadCols
    (test_gpu_truth.test_bipolar_quadrature_vs_truth); none when every column is evaluated."""
    Ni, Nj, lat0 = int(s["params"][0]), int(s["params"][1]), float(s["params"][2])
    zq, jg = int(np.ceil(6.0 * Ni / 360.0)), qb.guard_row(Nj, lat0)
    image = {}
    for f, shp in s["shapes"].items():
        jj, ii = np.meshgrid(np.arange(shp[0]), np.arange(shp[1]), indexing="ij")
        image[f] = (jj < jg) & ~((ii < Ni // 4) | ((ii >= Ni // 2 - zq) & (ii < Ni // 2 + zq)) | (ii >= Ni - zq)) & bool(mirrored)
    return image


def _dpole_image(s, mirrored):
    """The other half of each row than the one the strips walk (test_gpu_truth.test_displaced_pole_quadrature_vs_truth)."""
    nx, lon0, lon_dp = int(s["params"][0]), float(s["params"][2]), float(s["params"][4])
    c0 = int(round(((lon_dp - lon0) % 360.0) * nx / 360.0)) % nx
    c0 = c0 - nx // 2 if c0 > nx // 2 else c0
    image = {}
    for f, shp in s["shapes"].items():
        ii = np.broadcast_to(np.arange(shp[1])[None, :], shp)
        image[f] = ~((ii >= c0) & (ii < c0 + nx // 2)) & bool(mirrored)
    return image


def _sym_id(sym):
    return "mirror" if sym else "every_column"


# ---------------------------------------------------------------------------------------------------------------
# the pass
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sym", SYMS)
@pytest.mark.parametrize("tag,dp_arc", [(t, None) for t in BIPOLAR] + [(t, a) for t in DPOLE for a in ("chord", "literal")])
def test_pass_metrics_vs_truth(ogg, tag, dp_arc, sym):
    kind, flags = CAPS[tag]
    s = qb.load(tag)
    par = s["params"]
    plan, fields = _pass_fields(dict(flags, **({"dp_arc": dp_arc} if dp_arc else {})), sym)
    if kind == "bipolar":
        Ni, Nj, lat0, lon_bp, rp = int(par[0]), int(par[1]), float(par[2]), float(par[3]), float(par[4])
        bp = next(b for b in plan.subs if b.name == "BP")
        assert (plan.Ni, bp.Nj) == (Ni, Nj) and bp.lat0_bp == lat0 and bp.lon_bp == lon_bp and abs(bp.rp - rp) < 1e-15      # lat0: the fixture's bits
        arrays = tuple(fields["BP"][f] for f in qb.FIELDS)
        image = _bipolar_image(s, sym)
    else:
        nx, ny, lon0, lat0, lon_dp, r_dp, row0, nrow = int(par[0]), int(par[1]), float(par[2]), float(par[3]), float(par[4]), float(par[5]), int(par[6]), int(par[7])
        sc = plan.subs[0]
        assert sc.kind == "dpole" and (plan.Ni, sc.Nj) == (nx, ny) and sc.row0 <= row0 and sc.row0 + sc.nj1 == row0 + nrow == ny + 1
        assert sc.lat0 == lat0 and sc.lon_dp == lon_dp and plan.lon0 == lon0 and abs(sc.r_dp - r_dp) < 1e-15                    # lat0: the fixture's bits
        arrays = tuple(fields["SC"][f][row0 - sc.row0:] for f in qb.FIELDS)
        image = _dpole_image(s, sym and dp_arc == "chord")
    _held("%s/pass%s/%s" % (tag.rstrip("_"), "_" + dp_arc if dp_arc else "", _sym_id(sym)), arrays, tag, image=image)


# ---------------------------------------------------------------------------------------------------------------
# the function-level entry points
# ---------------------------------------------------------------------------------------------------------------
def _bipolar_function(ogg, monkeypatch, s, order, guard_k, sym):
    par = s["params"]
    if guard_k is not None:
        monkeypatch.setenv("OGG_BP_GUARD_K", guard_k)
    return ogg.bipolar_cap_metrics_quad_fast(order, int(par[0]), int(par[1]), float(par[2]), float(par[3]), float(par[4]), symmetry=sym)


def _dpole_function(ogg, s, order, arc, sym):
    par = s["params"]
    kw = {"symmetry": sym} if arc == "chord" else {}
    got = ogg.displacedPoleCap_metrics_quad(order, int(par[0]), int(par[1]), float(par[2]), float(par[3]), float(par[4]), float(par[5]), arc_form=arc, **kw)
    return tuple(np.ascontiguousarray(a[int(par[6]):]) for a in got)


@pytest.mark.parametrize("sym", SYMS)
@pytest.mark.parametrize("guard_k", [None, "0"])
@pytest.mark.parametrize("tag", BIPOLAR)
def test_bipolar_function_metrics_vs_truth(ogg, monkeypatch, tag, guard_k, sym):
    s = qb.load(tag)
    arrays = _bipolar_function(ogg, monkeypatch, s, 5, guard_k, sym)
    _held("%s/functions%s/%s" % (tag.rstrip("_"), "" if guard_k is None else "_every_cell_literal", _sym_id(sym)), arrays, tag,
          image=_bipolar_image(s, sym and guard_k is None))


@pytest.mark.parametrize("arc,sym", [("literal", None), ("chord", True), ("chord", False)])
@pytest.mark.parametrize("tag", DPOLE)
def test_displaced_pole_function_metrics_vs_truth(ogg, tag, arc, sym):
    s = qb.load(tag)
    arrays = _dpole_function(ogg, s, 4, arc, sym)
    _held("%s/functions_%s%s" % (tag.rstrip("_"), arc, "" if sym is None else "/" + _sym_id(sym)), arrays, tag, image=_dpole_image(s, bool(sym)))


@pytest.mark.parametrize("sym", SYMS)
@pytest.mark.parametrize("guard_k", [None, "0"])
@pytest.mark.parametrize("order", qb.REDUCED_ORDERS["sbp180_"])
def test_bipolar_function_other_orders_vs_truth(ogg, monkeypatch, order, guard_k, sym):
    """Orders 2, 3, 4 on the bottom cell row, a mid-cap row and every row from the guard's first row - 1 up (and the top edge row of dx)."""
    s = qb.load("sbp180_", order)
    arrays = _bipolar_function(ogg, monkeypatch, s, order, guard_k, sym)
    _held("sbp180/functions%s_order%d/%s" % ("" if guard_k is None else "_every_cell_literal", order, _sym_id(sym)), arrays, "sbp180_", order=order,
          image=_bipolar_image(s, sym and guard_k is None))


@pytest.mark.parametrize("arc,sym", [("literal", None), ("chord", True), ("chord", False)])
@pytest.mark.parametrize("order", qb.REDUCED_ORDERS["sdp_rdp_"])
def test_displaced_pole_function_other_orders_vs_truth(ogg, order, arc, sym):
    """Order 2 (quadrature and central differences) on the first, a middle and the last kept cell row (and the top edge row of dx)."""
    s = qb.load("sdp_rdp_", order)
    arrays = _dpole_function(ogg, s, order, arc, sym)
    _held("sdp_rdp/functions_%s_order%d%s" % (arc, order, "" if sym is None else "/" + _sym_id(sym)), arrays, "sdp_rdp_", order=order,
          image=_dpole_image(s, bool(sym)))
