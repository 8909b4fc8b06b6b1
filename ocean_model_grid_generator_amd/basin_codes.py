"""Basin codes: the integer basin of every wet model cell (Southern Ocean, Atlantic, Pacific, Arctic, ...), as MOM6 set-ups keep it
in basin_codes.nc for overturning and heat transport by basin, regional restoring and analysis masks.  include/ogg_hip.h, "Basin
codes", gives the definition; the reference has no such step.

An ordered list of rules, each a seeded flood confined to a longitude / latitude box: rule k takes the connected wet cells around its
seed that lie in its box and that no earlier rule took.  Several rules may share a code.  The floods run on the device
(ogg_basin_codes_dev, or the host-pointer ogg_basin_codes) as connected components under a per-cell class, on the ocean mask's
union-find; consecutive rules with disjoint boxes run as one pass.  Every output is an integer, so every path, knob and rank count
writes the same bytes.  No table of rules ships with the package: a rule file is written for the grid and the coastline at hand.

A rule file holds one rule per line, ``#`` starts a comment:

    code seed_lon seed_lat lon_w lon_e lat_s lat_n [name]

    python -m ocean_model_grid_generator_amd.basin_codes ocean_hgrid.nc (--topog topog.nc | --mask ocean_mask.nc) --rules FILE
        [--seed_max_km D] -o basin_codes.nc [--json summary.json]
"""
import argparse
import ctypes
import json
import sys

import numpy as np

from . import _lib as L
from . import exchange_grid as X
from . import fields as F
from . import netcdf3

N_LISTED = 10          # uncoded bodies of water listed in the summary (largest first)
REASONS = {L.BASIN_SEED_LAND: "the seed cell is land", L.BASIN_SEED_OUTSIDE: "the seed cell's centre is outside the box",
           L.BASIN_SEED_CODED: "the seed cell was taken by rule %d", L.BASIN_SEED_OFF_GRID: "the seed is off the grid",
           L.BASIN_SEED_INVALID: "the grid has no valid cell"}
RULE_FIELDS = ("code", "seed_lon", "seed_lat", "lon_w", "lon_e", "lat_s", "lat_n")


# ---- rules -----------------------------------------------------------------------------------------------------
class Rules(object):
    """The ordered rules as the library takes them (``table``: L.BASIN_RULE records) and the name of each (None without one)"""

    def __init__(self, table, names):
        self.table, self.names = table, list(names)

    def __len__(self):
        return self.table.shape[0]


def rules_of(rules):
    """Rules from a Rules, or from rows (code, seed_lon, seed_lat, lon_w, lon_e, lat_s, lat_n[, name])"""
    if isinstance(rules, Rules):
        return rules
    rows = [tuple(r) for r in rules]
    t = np.zeros(len(rows), dtype=L.BASIN_RULE)
    names = []
    for k, r in enumerate(rows):
        if len(r) not in (7, 8):
            raise ValueError("basin codes: rule %d has %d values: code seed_lon seed_lat lon_w lon_e lat_s lat_n [name]" % (k, len(r)))
        code = float(r[0])
        if not (np.isfinite(code) and code == int(code) and abs(code) < 2 ** 31):   # (a NaN too; the range 1 .. 255 is the library's check)
            raise ValueError("basin codes: rule %d: the code %r is not an integer" % (k, r[0]))
        t[k] = (int(code), 0) + tuple(float(v) for v in r[1:7])
        names.append(str(r[7]) if len(r) == 8 and r[7] is not None else None)
    return Rules(t, names)


def read_rules(path):
    """The rules of a text file: one rule per line, ``code seed_lon seed_lat lon_w lon_e lat_s lat_n [name]``; ``#`` starts a
    comment; rules that share a code share its name (a code with two names is refused)."""
    rows, named = [], {}
    with open(path) as fh:
        for no, line in enumerate(fh, 1):
            w = line.split("#", 1)[0].split()
            if not w:
                continue
            if len(w) not in (7, 8):
                raise ValueError("%s:%d: %d values: code seed_lon seed_lat lon_w lon_e lat_s lat_n [name]" % (path, no, len(w)))
            try:
                code = int(w[0])
                vals = [float(v) for v in w[1:7]]
            except ValueError:
                raise ValueError("%s:%d: an integer code and six numbers are needed: %s" % (path, no, " ".join(w)))
            name = w[7] if len(w) == 8 else None
            if name is not None and named.setdefault(code, name) != name:
                raise ValueError("%s:%d: code %d is named %s and %s" % (path, no, code, named[code], name))
            rows.append((code,) + tuple(vals) + (name,))
    if not rows:
        raise ValueError("%s: no rules" % path)
    return rules_of([r[:7] + (r[7] if r[7] is not None else named.get(r[0]),) for r in rows])


def seed_max_d2(seed_max_distance, Re=X.DEFAULT_RE):
    """the squared chord of a distance in metres: (2 sin(s / (2 Re)))^2; None: +inf (off)"""
    if seed_max_distance is None:
        return float("inf")
    s = float(seed_max_distance)
    if not (s >= 0.0):
        raise ValueError("basin codes: seed_max_distance must be >= 0 (%r)" % (seed_max_distance,))
    return float((2.0 * np.sin(min(s / (2.0 * Re), 0.5 * np.pi))) ** 2)


def params(ny, nx, rules, periodic=False, fold=False, seed_max_distance=None, Re=X.DEFAULT_RE):
    """an ogg_basin_params, checked with the rules by the library (OGG_EARG -> ValueError)"""
    from . import ocean_mask as M
    p = L.BasinParams(ny=int(ny), nx=int(nx), topology=M.topology_flags(periodic, fold), n_rules=len(rules),
                      seed_max_d2=seed_max_d2(seed_max_distance, Re))
    return L.checked("ogg_basin_check", p, rules.table.ctypes.data)


def plan(rules):
    """the passes of the rules: [first rule of each pass] + [K] (ogg_basin_plan; OGG_BASIN_BATCH=0: one rule per pass)"""
    rules = rules_of(rules)
    p = params(1, 1, rules)
    start = np.zeros(len(rules) + 1, dtype=np.int32)
    n = ctypes.c_int(0)
    L.call("ogg_basin_plan", ctypes.byref(p), rules.table.ctypes.data, start.ctypes.data, ctypes.byref(n))
    return [int(v) for v in start[:n.value + 1]]


# ---- the result ------------------------------------------------------------------------------------------------
def uncoded_bodies(plane, periodic, fold):
    """the connected bodies of a plane (1.0: wet and uncoded) by the ocean mask's label step on the current device: (number of
    bodies, [(cells, root)] of the N_LISTED largest)"""
    import torch
    from . import ocean_mask as M
    ny, nx = plane.shape
    dev = torch.device("cuda", torch.cuda.current_device())
    p = M.params(ny, nx, periodic, fold)
    d = torch.from_numpy(np.ascontiguousarray(plane, dtype=np.float64)).to(dev)
    wsb = int(L.load().ogg_mask_workspace_bytes(ctypes.byref(p)))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    root = torch.empty((ny, nx), dtype=torch.int32, device=dev)
    comps = torch.empty(ny * nx, dtype=torch.int64, device=dev)
    counts = torch.zeros(len(L.MASK_COUNT_FIELDS), dtype=torch.int64, device=dev)
    L.call("ogg_mask_label_dev", ctypes.byref(p), d.data_ptr(), ws.data_ptr(), wsb, root.data_ptr(), comps.data_ptr(), counts.data_ptr(),
           torch.cuda.current_stream(dev).cuda_stream)
    n = L.counts_dict(L.MASK_COUNT_FIELDS, counts)["components"]
    top = np.sort(comps[:n].cpu().numpy())[::-1][:N_LISTED]
    return n, [(int(c >> 32), int(np.iinfo(np.int32).max - (c & 0xFFFFFFFF))) for c in top]


def result(code, rule, records, counts, wet, rules, x, y, periodic, fold, seed_max_distance, Re, area=None):
    """What basin_codes() returns: code (uint8, 0: land or uncoded), rule (int16, -1 where code is 0), wet (uint8), records (one
    L.BASIN_RECORD per rule), counts, rules and a summary.  x, y: the supergrid points, numpy arrays or device tensors (only the
    listed bodies' centres are read).  area: None or the model-cell area (ny, nx), for the area per code."""
    ny, nx = code.shape
    cells = np.bincount(code.reshape(-1), minlength=256)
    areas = None if area is None else np.bincount(code.reshape(-1), weights=np.asarray(area, dtype=np.float64).reshape(-1), minlength=256)
    name_of = {}
    for k in range(len(rules)):
        name_of.setdefault(int(rules.table["code"][k]), rules.names[k])
    codes = [{"code": c, "name": name_of[c], "cells": int(cells[c]), "area_m2": None if areas is None else float(areas[c])}
             for c in sorted(name_of)]
    rr = [{"rule": k, "code": int(rules.table["code"][k]), "name": rules.names[k], "seed_cell": int(r["seed_cell"]),
           "status": int(r["status"]), "blocking_rule": int(r["blocking_rule"]), "cells": int(r["cells"])}
          for k, r in enumerate(records)]
    bodies, n_bodies = [], 0
    if counts["uncoded"] > 0:
        n_bodies, top = uncoded_bodies(((wet != 0) & (code == 0)).astype(np.float64), periodic, fold)
        for n, r in top:
            j, i = divmod(r, nx)
            lon, lat = float(x[2 * j + 1, 2 * i + 1]), float(y[2 * j + 1, 2 * i + 1])
            bodies.append({"cells": n, "root": r, "j": j, "i": i, "lon": lon if np.isfinite(lon) else None,
                           "lat": lat if np.isfinite(lat) else None})   # (an invalid centre has no place)
    summary = dict(counts, shape=[ny, nx], periodic=bool(periodic), fold=bool(fold), Re=float(Re), n_rules=len(rules),
                   seed_max_distance=None if seed_max_distance is None else float(seed_max_distance), codes=codes, rules=rr,
                   uncoded_bodies=n_bodies, uncoded_largest=bodies)
    return {"code": code, "rule": rule, "wet": np.ascontiguousarray(wet, dtype=np.uint8), "records": records, "counts": counts,
            "rule_table": rules, "summary": summary}


# ---- host arrays -----------------------------------------------------------------------------------------------
def basin_codes(x, y, wet, rules, periodic=None, fold=None, seed_max_distance=None, Re=X.DEFAULT_RE, area=None):
    """The basin codes of the model cells of a stitched supergrid x, y ((2 ny + 1) x (2 nx + 1), degrees) with the wet set ``wet``
    (one value per model cell, 0: land) under ``rules`` (a Rules, read_rules(), or rows), on one GPU through the host-pointer entry
    ogg_basin_codes.  periodic, fold: None to read them from the grid (ocean_mask.detect_topology).  seed_max_distance: metres beyond
    which a seed is off the grid (None: any distance).  A dict: see result()."""
    from . import ocean_mask as M
    rules = rules_of(rules)
    x, y = L.as_f64(x), L.as_f64(y)
    nyp, nxp = x.shape
    X.check_grid(nyp, nxp)
    shape = ((nyp - 1) // 2, (nxp - 1) // 2)
    m = F.wet_mask(wet, shape, "basin codes")
    p = params(shape[0], shape[1], rules, False, False, seed_max_distance, Re)   # the rules' refusals come before the grid's
    periodic, fold = F.resolve_topology(periodic, fold, lambda: M.detect_topology(x, y, 2))
    p = params(shape[0], shape[1], rules, periodic, fold, seed_max_distance, Re)
    code = np.empty(shape, np.uint8)
    rule = np.empty(shape, np.int16)
    rec = np.zeros(len(rules), dtype=L.BASIN_RECORD)
    c = L.BasinCounts()
    L.call("ogg_basin_codes", ctypes.byref(p), rules.table.ctypes.data, x.ctypes.data, y.ctypes.data, m.ctypes.data, code.ctypes.data,
           rule.ctypes.data, rec.ctypes.data, ctypes.byref(c))
    counts = L.counts_dict(L.BASIN_COUNT_FIELDS, c)
    return result(code, rule, rec, counts, m, rules, x, y, periodic, fold, seed_max_distance, Re, area)


# ---- device arrays ---------------------------------------------------------------------------------------------
def basin_codes_dev(x, y, wet, rules, periodic=None, fold=None, seed_max_distance=None, Re=X.DEFAULT_RE, area=None):
    """basin_codes() on one GPU with the grid x, y ((2 ny + 1) x (2 nx + 1)) as float64 device tensors: every pass on the device's
    current stream, without a host round trip between them.  The same dict as basin_codes(), with host arrays."""
    import torch
    from . import ocean_mask as M
    rules = rules_of(rules)
    dev = x.device
    x, y = x.contiguous(), y.contiguous()
    nyp, nxp = x.shape
    X.check_grid(nyp, nxp)
    shape = ((nyp - 1) // 2, (nxp - 1) // 2)
    m = F.wet_mask(wet.cpu().numpy() if hasattr(wet, "cpu") else wet, shape, "basin codes")
    p = params(shape[0], shape[1], rules, False, False, seed_max_distance, Re)
    periodic, fold = F.resolve_topology(periodic, fold, lambda: M.topology_of_device_grid(x, y))
    p = params(shape[0], shape[1], rules, periodic, fold, seed_max_distance, Re)
    st = torch.cuda.current_stream(dev).cuda_stream
    wsb = int(L.load().ogg_basin_workspace_bytes(ctypes.byref(p)))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    wt = torch.from_numpy(m).to(dev)
    rt = torch.from_numpy(rules.table.view(np.uint8)).to(dev)
    code = torch.empty(shape, dtype=torch.uint8, device=dev)
    rule = torch.empty(shape, dtype=torch.int16, device=dev)
    rec = torch.empty(len(rules) * L.BASIN_RECORD.itemsize, dtype=torch.uint8, device=dev)
    counts = torch.zeros(len(L.BASIN_COUNT_FIELDS), dtype=torch.int64, device=dev)
    L.call("ogg_basin_codes_dev", ctypes.byref(p), rules.table.ctypes.data, rt.data_ptr(), x.data_ptr(), y.data_ptr(), nxp, wt.data_ptr(),
           ws.data_ptr(), wsb, code.data_ptr(), rule.data_ptr(), rec.data_ptr(), counts.data_ptr(), st)
    cd = L.counts_dict(L.BASIN_COUNT_FIELDS, counts)
    records = rec.cpu().numpy().view(L.BASIN_RECORD).copy()
    if area is not None and hasattr(area, "cpu"):
        area = area.cpu().numpy()
    return result(code.cpu().numpy(), rule.cpu().numpy(), records, cd, m, rules, x, y, periodic, fold, seed_max_distance, Re, area)


# ---- files -----------------------------------------------------------------------------------------------------
def write_basin_codes(path, res, title="basin codes of the model cells"):
    """basin (int, CF flag_values / flag_meanings from the rules' names), rule (short, -1 where basin is 0) and wet (byte), dims
    (ny, nx), as a NetCDF 64-bit-offset file; the rules as global attributes"""
    ny, nx = res["code"].shape
    s, rules = res["summary"], res["rule_table"]
    gatts = [("title", title), ("cells", "MOM6 model (h) cells: 2 x 2 supergrid cells"), ("periodic", int(s["periodic"])),
             ("fold", int(s["fold"])), ("n_rules", len(rules)), ("rule_columns", " ".join(RULE_FIELDS) + " name")]
    if s["seed_max_distance"] is not None:
        gatts.append(("seed_max_distance", float(s["seed_max_distance"])))
    for k in range(len(rules)):
        r = rules.table[k]
        gatts.append(("rule_%04d" % k, " ".join([str(int(r["code"]))] + [repr(float(r[f])) for f in RULE_FIELDS[1:]] +
                                                ([rules.names[k]] if rules.names[k] else []))))
    ds = netcdf3.Dataset(path, [("ny", ny), ("nx", nx)], global_atts=gatts)
    codes = [c["code"] for c in s["codes"]]
    atts = [("long_name", "basin code: 0 land or no basin"), ("flag_values", np.array([0] + codes, dtype=np.int32)),
            ("flag_meanings", " ".join(["none"] + [(c["name"] or "code_%d" % c["code"]) for c in s["codes"]]))]
    ds.def_var("basin", netcdf3.NC_INT, ("ny", "nx"), atts, res["code"].astype(np.int32))
    ds.def_var("rule", netcdf3.NC_SHORT, ("ny", "nx"), [("long_name", "index of the rule that took the cell, -1 where basin is 0")],
               res["rule"])
    ds.def_var("wet", netcdf3.NC_BYTE, ("ny", "nx"), [("long_name", "1 wet, 0 land")], res["wet"].astype(np.int8))
    ds.write()


def summary_lines(res):
    s = res["summary"]
    topo = ", ".join([t for t, f in (("periodic", s["periodic"]), ("folded", s["fold"])) if f]) or "neither periodic nor folded"
    out = ["   basin codes: %d x %d cells (%s): %d rules in %d passes coded %d of %d wet cells"
           % (s["shape"][1], s["shape"][0], topo, s["n_rules"], s["passes"], s["coded"], s["wet"])]
    for c in s["codes"]:
        area = "" if c["area_m2"] is None else ", %.6e m2" % c["area_m2"]
        out.append("   basin codes: code %d%s: %d cells%s" % (c["code"], " (%s)" % c["name"] if c["name"] else "", c["cells"], area))
    for r in s["rules"]:
        if r["status"] != L.BASIN_TOOK:
            why = REASONS[r["status"]]
            out.append("   basin codes: rule %d (code %d) took nothing: %s" % (r["rule"], r["code"],
                                                                             why % r["blocking_rule"] if "%d" in why else why))
    out.append("   basin codes: %d wet cells in %d bodies of water have no code" % (s["uncoded"], s["uncoded_bodies"]))
    for b in s["uncoded_largest"]:
        place = "an invalid centre" if b["lon"] is None or b["lat"] is None else "lon %.4f, lat %.4f" % (b["lon"], b["lat"])
        out.append("   basin codes: an uncoded body of %d cells at %s (cell j=%d, i=%d)" % (b["cells"], place, b["j"], b["i"]))
    return out


def main(argv=None):
    from . import remap as R
    from . import runoff as RO
    p = argparse.ArgumentParser(prog="python -m ocean_model_grid_generator_amd.basin_codes",
                                description="basin codes of the model cells of a supergrid file by ordered seeded floods")
    p.add_argument("grid", help="ocean_hgrid.nc (NetCDF classic / 64-bit offset)")
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--topog", default=None, help="topog.nc: cells with depth > 0 are wet")
    g.add_argument("--mask", default=None, help="ocean_mask.nc: cells with mask != 0 are wet")
    p.add_argument("--rules", required=True, help="the rule file: code seed_lon seed_lat lon_w lon_e lat_s lat_n [name] per line")
    p.add_argument("--seed_max_km", type=float, default=None, help="a seed farther than this from every cell centre is off the grid")
    p.add_argument("-o", "--output", default="basin_codes.nc")
    p.add_argument("--json", default=None, help="write the summary as JSON to this file")
    a = p.parse_args(argv)
    rules = read_rules(a.rules)
    h = netcdf3.read_header(a.grid)
    grid = netcdf3.read_doubles(a.grid, names=("x", "y") + (("area",) if "area" in h.vars else ()))
    res = basin_codes(grid["x"], grid["y"], R.mask_from_file(a.topog or a.mask), rules,
                      seed_max_distance=None if a.seed_max_km is None else 1000.0 * a.seed_max_km,
                      area=RO.cell_area(grid["area"]) if "area" in grid else None)
    for line in summary_lines(res):
        print(line)
    write_basin_codes(a.output, res)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res["summary"], fh, indent=1)
    return res


if __name__ == "__main__":
    main()
    sys.exit(0)
