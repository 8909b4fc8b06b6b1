"""EVERY dx, dy and area of a whole small cap against the 50-digit truth (plain numpy; used by tests/test_quad_bounds_cpu.py, by
tests/test_gpu_small_caps_metrics_truth.py and -- for the class masks only -- by scripts/truth_table.py --groups small_metrics).

The fixtures tests/golden/truth_small_caps_metrics*.npz hold, for the four caps of scripts/truth_table.py's SMALL_CAPS, the exact value of
the reference's quadrature at every element of the three arrays (bipolar: dx (Nj+1, Ni) with the top edge row, dy (Nj, Ni+1) with the last
column, area (Nj, Ni); displaced pole: the rows main() keeps, same shapes), as ONE 64-bit integer k per value, truth = k * 2^-bits with one
`bits` per cap and field, and the oracle's own distance from that truth per cap, field and class (`*_eref_rel_*`, `*_eref_abs_*`).

Classes come from the REFERENCE's conditioning only (the code under test has no say in them):

  bipolar   `pole`     the four cells of the top cell row that touch a pole point (columns Ni/4 - 1, Ni/4, 3Ni/4 - 1, 3Ni/4): acos(A) at
                       A -> 1 behind the j = ny - 0.001 node of OGG:146-147
            `edge`     within 6 columns of Ni/4 or 3Ni/4, or next to the fold lines (columns 0, 1, Ni/2 - 1 .. Ni/2 + 1, Ni - 2 ..): the
                       cancellation 1 - cos^2 of OGG:82-84
            `regular`  the rest
            (scripts/truth_table.py's bq_group, applied to the element's own (row, column); dx's top edge row and dy's last column are
            classed by their column like any other)
            `fold`     the values that VANISH on the fold lines, |truth| <= 1e-6 * max|truth| of the field (dy at columns 0, Ni/2, Ni): held
                       to 1e-6 m ABSOLUTE, the project's rule, and left out of the three relative classes
  dpole     `all`      one class per field; the two truths A (exact probe positions) and B (fp64-rounded probe positions) each have their
                       own measured distance

Bound of an element: K_REF * max(eref of its class, floor) relative to |truth|, with K_REF = 1.5 (tests/test_gpu_truth.py) and the floor
2e-14 for the bipolar quadrature (the project's value, test_bipolar_quadrature_vs_truth) and none for the displaced-pole quadrature.
A NaN is a failure.
"""
import os

import numpy as np

from test_gpu_truth import K_REF

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = {"sbp180_": "truth_small_caps_metrics.npz", "sbp360_": "truth_small_caps_metrics_sbp360.npz",
         "sdp_rdp_": "truth_small_caps_metrics_sdp_rdp.npz", "sdp_latdp_": "truth_small_caps_metrics_sdp_latdp.npz"}
KIND = {"sbp180_": "bipolar", "sbp360_": "bipolar", "sdp_rdp_": "dpole", "sdp_latdp_": "dpole"}
MAIN_ORDER = {"bipolar": 5, "dpole": 4}
REDUCED_ORDERS = {"sbp180_": (2, 3, 4), "sdp_rdp_": (2,)}
FIELDS = ("dx", "dy", "area")
FLOOR_REL = {"bipolar": 2e-14, "dpole": 0.0}
FOLD_REL, FOLD_ABS = 1e-6, 1e-6                    # |truth| <= FOLD_REL * max: compared absolutely, to FOLD_ABS metres
MAX_FILE_BYTES = 657155                            # tests/golden/truth_small_caps.npz


def scalar(a):
    """A stored scalar (the reproducible writer stores them with one element)."""
    return np.asarray(a).reshape(-1)[0]


def pairs(k, bits):
    """The fixture's integers (truth = k 2^-bits) as (..., 2) hi / lo pairs: hi = fp64(k 2^-bits), lo = the rest, exactly."""
    k = np.asarray(k, dtype=np.int64)
    hi = np.ldexp(k.astype(np.float64), -int(bits))
    rest = k - np.ldexp(hi, int(bits)).astype(np.int64)
    return np.stack([hi, np.ldexp(rest.astype(np.float64), -int(bits))], axis=-1)


def err(v, t):
    """|v - truth| with truth = t[..., 0] + t[..., 1]."""
    return np.abs((np.asarray(v, dtype=np.float64) - t[..., 0]) - t[..., 1])


def guard_row(Nj, lat0):
    """The first cell row of the bipolar quadrature's exactness guard (tests/test_gpu_truth.py::test_bipolar_quadrature_vs_truth)."""
    return int(np.floor(Nj * (np.degrees(np.arccos(2.0 / np.sqrt(4000.0))) - lat0) / (90.0 - lat0))) - 1


def classes(kind, shape, Ni, n_cell_rows):
    """{class: boolean mask of `shape`} from the element's own (row, column): a partition."""
    jj, ii = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), indexing="ij")
    if kind != "bipolar":
        return {"all": np.ones(shape, bool)}
    q = Ni // 4
    pole = (jj == n_cell_rows - 1) & np.isin(ii, (q - 1, q, 3 * q - 1, 3 * q))
    edge = ((np.abs(ii - q) <= 6) | (np.abs(ii - 3 * q) <= 6) | (np.abs(ii - Ni // 2) <= 1) | (ii <= 1) | (ii >= Ni - 2)) & ~pole
    return {"regular": ~pole & ~edge, "edge": edge, "pole": pole}


def fold(t_hi):
    """The values that vanish on the fold lines: |truth| <= FOLD_REL * max|truth| (from the TRUTH alone)."""
    a = np.abs(t_hi)
    return a <= FOLD_REL * a.max()


def shapes(kind, par):
    """(dx, dy, area) shapes of the cap's arrays from the fixture's parameters."""
    Ni = int(par[0])
    nrow = int(par[1]) + 1 if kind == "bipolar" else int(par[7])
    return {"dx": (nrow, Ni), "dy": (nrow - 1, Ni + 1), "area": (nrow - 1, Ni)}


def oracle_arrays(tag, order=None):
    """The oracle's whole (dx, dy, area) of the cap from the fixture's parameters (the rows main() keeps); fresh, writable arrays."""
    from oracle import ogg_oracle as orc
    s = load(tag, order)
    par = s["params"]
    if s["kind"] == "bipolar":
        return orc.bipolar_cap_metrics_quad_fast(s["order"], int(par[0]), int(par[1]), float(par[2]), float(par[3]), float(par[4]))
    row0 = int(par[6])
    o = orc.displacedPoleCap_metrics_quad(s["order"], int(par[0]), int(par[1]), float(par[2]), float(par[3]), float(par[4]), float(par[5]), j_first=row0)
    return tuple(np.ascontiguousarray(a[row0:]) for a in o)


class QuadBoundError(AssertionError):
    """check() failed; `.worst` = the five worst elements as (truth, field, j, i, distance, bound), worst first; `.rep` = what check()
    would have returned."""

    def __init__(self, msg, worst, rep):
        super().__init__(msg)
        self.worst, self.rep = worst, rep


_CACHE = {}


def load(tag, order=None):
    """One truth set of one cap: {"kind", "params", "order", "shapes", "rows" (cell rows held), "dx_rows" (rows of dx held), "truths":
    {"" | "A" | "B": {field: (n_rows_held, ncol, 2) hi / lo pairs}}, "bits": {field: b}, "eref": {(T, field, class, "rel" | "abs"): value},
    "census": {(field, class): n}}.  `order` None: the order main() uses (5 / 4), every row; else a reduced-row set."""
    kind = KIND[tag]
    if tag not in _CACHE:
        _CACHE[tag] = dict(np.load(os.path.join(GOLD, FILES[tag])).items())
    z = _CACHE[tag]
    if order is None or order == MAIN_ORDER[kind]:
        p, order = tag, MAIN_ORDER[kind]
    else:
        p = "%so%d_" % (tag, order)
    par = z[tag + "params"]
    Ts = ("",) if kind == "bipolar" else ("A", "B")
    s = {"kind": kind, "params": par, "order": int(scalar(z[p + "order"])), "shapes": shapes(kind, par), "rows": z[p + "rows"], "dx_rows": z[p + "dx_rows"],
         "bits": {f: int(scalar(z[p + f + "_bits"])) for f in FIELDS}, "truths": {}, "eref": {}, "census": {}, "prefix": p}
    assert s["order"] == order
    for T in Ts:
        s["truths"][T] = {f: pairs(z[p + (T + "_" if T else "") + f], s["bits"][f]) for f in FIELDS}
    for key in z:
        if key.startswith(p) and "_eref_" in key and (p != tag or not key[len(p):].startswith("o")):
            head, cls = key[len(p):].split("_eref_")
            how, cls = cls.split("_", 1)
            T, f = (head.split("_") if "_" in head else ("", head))
            s["eref"][T, f, cls, how] = float(scalar(z[key]))
        if key.startswith(p) and "_census_" in key and (p != tag or not key[len(p):].startswith("o")):
            f, cls = key[len(p):].split("_census_")
            s["census"][f, cls] = int(scalar(z[key]))
    return s


def element_bounds(s, T, field):
    """(rel, fold_mask, class_masks) on the HELD rows of `field`: rel = the relative bound of every element (K_REF * max(eref, floor));
    fold_mask = the elements compared absolutely instead."""
    rows = s["dx_rows"] if field == "dx" else s["rows"]
    t = s["truths"][T][field]
    Ni = int(s["params"][0])
    cl = {nm: m[rows] for nm, m in classes(s["kind"], s["shapes"][field], Ni, s["shapes"]["area"][0]).items()}
    fm = fold(t[..., 0])
    rel = np.zeros(t.shape[:-1])
    for nm, m in cl.items():
        if (T, field, nm, "rel") in s["eref"]:
            rel[m] = K_REF * max(s["eref"][T, field, nm, "rel"], FLOOR_REL[s["kind"]])
        else:
            assert not (m & ~fm).any(), (field, nm)           # a class without a measured distance holds fold values only
    return rel, fm, cl


def smallest_bound(s, T, field):
    """The smallest absolute bound any element of the field is held to (metres or square metres): what the fixture's unit must resolve."""
    rel, fm, _ = element_bounds(s, T, field)
    b = np.where(fm, FOLD_ABS, rel * np.abs(s["truths"][T][field][..., 0]))
    return float(b.min())


def check(dx, dy, area, tag, order=None, image=None, name=""):
    """Hold the three arrays (the cap's whole arrays, in the fixture's shapes) to the truth set (tag, order) at every element it holds.
    `image`: optional {field: boolean mask of the field's shape}, the elements whose value is a mirror image; they are reported as lines of
    their own ("<class>@image") and held to the same bound as their class.  Returns {"[A/|B/]field/class": {"oracle_vs_truth", "vs_truth",
    "bound", "n"}} -- relative distances, absolute (metres) for the class "fold".  Raises AssertionError naming the five worst elements
    (truth, field, j, i, distance, bound) if any element exceeds its bound or is not finite."""
    s = load(tag, order)
    got = {"dx": np.asarray(dx), "dy": np.asarray(dy), "area": np.asarray(area)}
    rep, bad = {}, []
    for T in s["truths"]:
        for f in FIELDS:
            assert got[f].shape == s["shapes"][f], (name, f, got[f].shape, s["shapes"][f])
            rows = s["dx_rows"] if f == "dx" else s["rows"]
            t = s["truths"][T][f]
            rel, fm, cl = element_bounds(s, T, f)
            e = err(got[f][rows], t)
            with np.errstate(divide="ignore", invalid="ignore"):
                d = np.where(fm, e, e / np.abs(t[..., 0]))                    # the distance in the unit of its bound
            d = np.where(np.isfinite(d), d, np.inf)                            # a NaN or inf in the field is a failure
            bound = np.where(fm, FOLD_ABS, rel)
            ratio = d / bound
            groups = [(nm, m & ~fm) for nm, m in cl.items()] + [("fold", fm)]
            if image is not None:
                im = np.asarray(image[f])[rows]
                groups += [(nm + "@image", m & im) for nm, m in groups]
            pre = (T + "/" if T else "") + f + "/"
            for nm, m in groups:
                if not m.any():
                    continue
                base = nm.split("@")[0]
                how = "abs" if base == "fold" else "rel"
                rep[pre + nm] = {"oracle_vs_truth": s["eref"].get((T, f, base, how), 0.0), "vs_truth": float(d[m].max()), "bound": float(bound[m].max()),
                                 "n": int(m.sum())}
            for k in np.argsort(ratio, axis=None)[::-1][:5]:
                j, i = np.unravel_index(k, ratio.shape)
                if ratio[j, i] > 1.0:
                    bad.append((float(ratio[j, i]), T, f, int(rows[j]), int(i), float(d[j, i]), float(bound[j, i])))
    if bad:
        bad.sort(reverse=True)
        worst = [b[1:] for b in bad[:5]]
        raise QuadBoundError("%s %s order %d: beyond the bound; five worst (truth, field, j, i, distance, bound): %s" % (name, tag, s["order"], worst), worst, rep)
    return rep
