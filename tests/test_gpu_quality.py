"""GPU tests of the grid-quality report (csrc/ogg_quality.hip, grid_quality.py, Supergrid.quality): against the numpy definition
in oracle/quality_oracle.py, the device pipeline against the host-array entry, independence of the band split, the joints, main()'s
--quality_report and the file checker."""
import json
import os

import numpy as np
import pytest

from oracle import quality_oracle as qo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RE = 6371.0e3


@pytest.fixture(scope="module")
def sg(hip):
    import ocean_model_grid_generator_amd.supergrid as m
    return m


def delta_tolerance(x, y):
    """Per corner: 1e-10 deg, or what a difference of two unit vectors carries when its chord is short.  P(j, i) has a rounding error
    of a few units of 2^-53 in the oracle (numpy's cos / sin of deg2rad) and in the kernel (sincospi): the chords A, B and the angle
    between them then carry ~ 2^-53 / |chord| radians, which exceeds 1e-10 deg for chords under ~ 1e-5 (60 m), e.g. next to the
    singular points of the caps."""
    P = qo.unit_vectors(x, y)
    p0 = P[:-1, :-1]
    short = np.minimum(np.linalg.norm(P[:-1, 1:] - p0, axis=-1), np.linalg.norm(P[1:, :-1] - p0, axis=-1))
    with np.errstate(divide="ignore"):
        return np.maximum(1e-10, np.degrees(64 * 2.0 ** -53 / short))


def check_against_oracle(got, want, x, y):
    """Sizes, ratios and aspect ratio bitwise with their locations; the largest delta within the tolerance of delta_tolerance (location
    equal, or the oracle's delta there within that tolerance of the maximum); bin counts equal except for corners within that
    tolerance of a bin edge."""
    for f in ("dx", "dy", "area"):
        if want[f] is None:
            assert got[f] is None
            continue
        assert got[f] == want[f], (f, got[f], want[f])
    for f in ("aspect_ratio_max", "rx_max", "ry_max"):
        assert got[f] == want[f], (f, got[f], want[f])
    gc, wc = got["corner"], want["corner"]
    assert gc["n"] == wc["n"] and gc["n_degenerate"] == wc["n_degenerate"]
    delta, tol = qo.corner_delta(x, y, RE), delta_tolerance(x, y)
    gm, wm = gc["delta_max_deg"], wc["delta_max_deg"]
    t = max(tol[gm["j"], gm["i"]], tol[wm["j"], wm["i"]])
    assert abs(gm["value"] - wm["value"]) <= t, (gm, wm, t)
    if (gm["j"], gm["i"]) != (wm["j"], wm["i"]):
        assert abs(delta[gm["j"], gm["i"]] - wm["value"]) <= t
    if gc["histogram"] != wc["histogram"]:
        ok = ~np.isnan(delta)
        d, tl = delta[ok], tol[ok]
        near = sum(int(np.sum(np.abs(d - e) <= tl)) for e in qo.BIN_EDGES_DEG)
        assert sum(abs(a - b) for a, b in zip(gc["histogram"], wc["histogram"])) <= 2 * near, (gc["histogram"], wc["histogram"])
    assert sum(gc["histogram"]) + gc["n_degenerate"] == gc["n"]


@pytest.mark.parametrize("fixture", ["ref_small_r0.25_even", "ref_small_r0.5_dp"])
def test_golden_fixtures_against_oracle(hip, fixture):
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    d = np.load(os.path.join(ROOT, "tests", "golden", fixture + ".npz"))
    f = [d[k] for k in ("x", "y", "dx", "dy", "area")]
    got = ogg.grid_quality(*f, Re=RE)
    check_against_oracle(got["grid"], qo.grid_section(*f, Re=RE), f[0], f[1])
    assert sorted(got) == ["Re", "corner_bin_edges_deg", "degenerate_m", "grid", "metrics", "nxp", "nyp"]


CONFIGS = {
    "r2": dict(inverse_resolution=2.0),
    "om4": dict(inverse_resolution=4.0, r_dp=0.2, south_cutoff_row=83),
    "r8_dp": dict(inverse_resolution=8.0, r_dp=0.2),
    "r8_dp_cut": dict(inverse_resolution=8.0, r_dp=0.2, south_cutoff_row=21),
    "r2_skip": dict(inverse_resolution=2.0, skip_metrics=True),
    "r8": dict(inverse_resolution=8.0),
}


def device_grid(sg, name, world=1, **kw):
    plan = sg.SupergridPlan(**CONFIGS[name], **kw)
    ranks = []
    for r in range(world):
        ranks.append(sg.Supergrid(plan, rank=r, world=world, device="cuda:0", halo="local", peers=ranks))
    for g in ranks:
        g.run_pass()
    return plan, ranks


def stitched(sg, plan, ranks):
    return sg.stitch(plan, [g.bands_to_host() for g in ranks])


def sections_of(out):
    names = [n for n in ("SC", "SO", "Merc", "BP") if n in out["sub"]]
    starts = list(np.cumsum([0] + [out["sub"][n]["x"].shape[0] - 1 for n in names[:-1]]))
    seams = [(out["sub"][n]["x"][-1], out["sub"][n]["y"][-1]) for n in names[:-1]]
    return list(zip(names, starts)), seams


@pytest.mark.parametrize("name", ["r2", "om4", "r8_dp"])
def test_stitched_grids_against_oracle(sg, name):
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    plan, ranks = device_grid(sg, name)
    out = stitched(sg, plan, ranks)
    f = [out[k] for k in ("x", "y", "dx", "dy", "area")]
    got = ogg.grid_quality(*f, Re=plan.Re)
    check_against_oracle(got["grid"], qo.grid_section(*f, Re=plan.Re), f[0], f[1])


@pytest.mark.parametrize("name", ["r2", "om4", "r8", "r8_dp", "r8_dp_cut", "r2_skip"])
def test_pipeline_report_equals_host_arrays(sg, name, tmp_path):
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    plan, ranks = device_grid(sg, name)
    g = ranks[0]
    cut = g.south_cut()
    rep = g.quality(cut)
    out = stitched(sg, plan, ranks)
    metrics = () if plan.skip_metrics else tuple(out[k] for k in ("dx", "dy", "area"))
    secs, seams = sections_of(out)
    host = ogg.grid_quality(out["x"], out["y"], *metrics, Re=plan.Re, sections=secs, seams=seams)
    assert rep == host
    assert rep["nyp"] == out["x"].shape[0]
    if plan.skip_metrics:
        assert rep["grid"]["dx"] is None and rep["grid"]["corner"]["delta_max_deg"] is not None
        assert all(j["ry"] is None and j["seam_m"] is not None for j in rep["joints"])


@pytest.mark.parametrize("name", ["r2", "om4"])
@pytest.mark.parametrize("world", [2, 3])
def test_report_is_independent_of_the_band_split(sg, name, world):
    plan1, one = device_grid(sg, name)
    want = one[0].quality(one[0].south_cut())
    plan, ranks = device_grid(sg, name, world=world)
    got = ranks[0].quality(ranks[0].south_cut())
    assert got == want


def test_joints_seams_and_match_dy(sg, capsys):
    for name in ("r2", "om4", "r8_dp"):
        plan, ranks = device_grid(sg, name)
        g = ranks[0]
        cut = g.south_cut()
        sg.check_guards(g.stitched_column("y", plan.Ni // 4, cut), any(s.name == "BP" for s in plan.subs))
        rep = g.quality(cut)
        assert len(rep["joints"]) == len(plan.subs) - (1 if cut[2] else 0) - 1
        for jt in rep["joints"]:
            assert jt["seam_m"]["value"] <= 1e-6, (name, jt)
    ratios = {}
    for match in ((), ("so",)):
        plan = sg.SupergridPlan(inverse_resolution=4.0, south_ocean_lower_lat=-88.57, no_south_cap=True, match_dy=match)
        g = sg.Supergrid(plan, device="cuda:0")
        g.run_pass()
        rep = g.quality(g.south_cut())
        jt = next(j for j in rep["joints"] if (j["lower"], j["upper"]) == ("SO", "Merc"))
        ratios[match] = jt["ry"]["value"]
    with capsys.disabled():
        print("\nSO/Merc joint dy ratio (-r 4 --south_ocean_lower_lat -88.57 --no_south_cap): without --match_dy so %.9f, with %.9f"
              % (ratios[()], ratios[("so",)]))
    assert ratios[("so",)] <= ratios[()]


def test_main_quality_report_and_file_checker(hip, tmp_path, capsys):
    from ocean_model_grid_generator_amd import grid_quality as Q
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    a, b, rp = str(tmp_path / "a.nc"), str(tmp_path / "b.nc"), str(tmp_path / "q.json")
    ogg.main(2.0, gridfilename=a, no_changing_meta=True)
    plain = capsys.readouterr().out
    ogg.main(2.0, gridfilename=b, no_changing_meta=True, quality_report=rp)
    with_q = capsys.readouterr().out
    assert open(a, "rb").read() == open(b, "rb").read()
    assert "grid quality" not in plain and "grid quality: max corner" in with_q
    rep = json.load(open(rp))
    rf = str(tmp_path / "qf.json")
    ogg.main(2.0, gridfilename=None, no_changing_meta=True, quality_report=rf, path="functions")
    assert json.load(open(rf)) == rep
    filerep = Q.main([b, "--json", str(tmp_path / "file.json")])
    assert json.loads(json.dumps(filerep["grid"])) == rep["grid"]
    assert json.load(open(str(tmp_path / "file.json")))["grid"] == rep["grid"]
