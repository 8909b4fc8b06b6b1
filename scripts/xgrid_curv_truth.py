#!/usr/bin/env python3
"""Extended-precision TRUTH for the curvilinear-source exchange grid's areas on the zoo of tests/xgrid_cs_definition.py under the
source meshes of tests/xgrid_curv_definition.py (sources_for).

CPU only (mpmath, 50 digits):

    python scripts/xgrid_curv_truth.py      ->  tests/golden/xgrid_curv_truth.npz

What "truth" means here: the statements of the definition (include/ogg_hip.h, "Exchange grid with a curvilinear source grid";
tests/xgrid_curv_definition.py) on the same fp64 corners, with every operation and every transcendental carried to 50 digits, pi
included, and rounded once at the end, in the manner of scripts/xgrid_truth.py and scripts/xgrid_cs_truth.py.  The candidates are
those of the fp64 boxes (the truth's corner vectors rounded to fp64).  |fp64 definition - truth| is the definition's own rounding
error, the yardstick the device is held to (tests/test_gpu_xgrid_curv.py): a kernel no further from the truth than 1.5 times that
cannot be told from the definition on another libm.

Stored, over every case "<zoo name>/<source name>": per case the range of its cells and pieces (cell_off, piece_off); a_poly (hi, lo)
of every model cell in row-major order (NaN where the cell is DEGENERATE or WIDE); pieces (I, J, n, m) of every entry kept at the
default threshold and area (hi, lo), with hi = fp64(truth) and lo = fp64(truth - hi); and the fp64 definition's distance from the
truth relative to A_poly, as measured when the file was made (eref_poly, eref_piece).
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import xgrid_cs_definition as cd  # noqa: E402
import xgrid_curv_definition as vd  # noqa: E402

mp.mp.dps = 50
OUT = os.path.join(ROOT, "tests", "golden", "xgrid_curv_truth.npz")
RE = 6371.0e3


class MP:
    """50 digits"""
    D = mp.pi / 180
    num = staticmethod(lambda v: mp.mpf(float(v)))
    cos, sin, sqrt, atan2 = mp.cos, mp.sin, mp.sqrt, mp.atan2


def split(t):
    if t is None:
        return np.nan, np.nan
    hi = float(t)
    return hi, float(t - mp.mpf(hi))


def table():
    names, cell_off, piece_off, a_poly, pieces, areas = [], [0], [0], [], [], []
    e_poly, e_piece = 0.0, 0.0
    for name, (x, y, _) in cd.zoo().items():
        for sname, (sx, sy) in vd.sources_for(x, y).items():
            lst, ap = vd.exchange_grid_curv(x, y, sx, sy, Re=RE, M=MP)[:2]
            dlst, dap = vd.exchange_grid_curv(x, y, sx, sy, Re=RE)[:2]
            names.append("%s/%s" % (name, sname))
            flat, dflat = [v for row in ap for v in row], [v for row in dap for v in row]
            a_poly += [split(v) for v in flat]
            cell_off.append(len(a_poly))
            for v, d in zip(flat, dflat):
                if v is not None and v > 0:
                    e_poly = max(e_poly, float(abs(mp.mpf(d) - v) / v))
            nx = len(ap[0])
            got = {e[:4]: e[4] for e in dlst}
            for e in lst:
                pieces.append(e[:4])
                areas.append(split(e[4]))
                if e[:4] in got:
                    e_piece = max(e_piece, float(abs(mp.mpf(got[e[:4]]) - e[4]) / flat[e[3] * nx + e[2]]))
            piece_off.append(len(pieces))
    return {"dps": np.array(mp.mp.dps), "cases": np.array(names), "cell_off": np.array(cell_off, np.int64),
            "piece_off": np.array(piece_off, np.int64), "a_poly": np.array(a_poly), "pieces": np.array(pieces, np.int32).reshape(-1, 4),
            "area": np.array(areas), "eref_poly": np.array(e_poly), "eref_piece": np.array(e_piece)}


def main():
    out = table()
    np.savez_compressed(OUT, **out)
    print("%d cases, %d cells, %d pieces; definition vs truth: A_poly %.3e, pieces %.3e of A_poly" % (
        out["cases"].size, out["a_poly"].shape[0], out["pieces"].shape[0], float(out["eref_poly"]), float(out["eref_piece"])))
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
