#!/usr/bin/env python3
"""Extended-precision TRUTH for the regional grids on the cases of tests/regional_definition.py (CASES).

CPU only (mpmath, 50 digits):

    python scripts/regional_truth.py      ->  tests/golden/regional_truth.npz

What "truth" means here: the statements of the definition (include/ogg_hip.h, "Regional grids"; tests/regional_definition.py) on the
same fp64 arguments, with every operation and every transcendental carried to 50 digits, pi included, and rounded once at the end, in
the manner of scripts/xgrid_curv_truth.py.  |fp64 definition - truth| is the definition's own rounding error, the yardstick the device
is held to (tests/test_gpu_regional.py): a kernel no further from the truth than 1.5 times that cannot be told from the definition on
another libm.

Stored: ``cases`` (the names, in the order of CASES); per case and field "<case>/<field>" the truth of the whole grid as an array
(2, rows, columns): hi = fp64(truth) and lo = fp64(truth - hi); and ``eref`` (cases x fields, the order of FIELDS): the fp64
definition's largest distance from the truth as measured when the file was made, in degrees for x, y, angle_dx and relative to the
truth for dx, dy, area.
"""
import os
import sys

import mpmath as mp
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import regional_definition as rd  # noqa: E402

mp.mp.dps = 50
OUT = os.path.join(ROOT, "tests", "golden", "regional_truth.npz")


def _mpf(v):
    return mp.mpf(float(v))


class MP:
    """50 digits, on numpy object arrays"""
    D = mp.pi / 180
    num = staticmethod(lambda v: np.frompyfunc(_mpf, 1, 1)(np.asarray(v, dtype=np.float64)))
    cos, sin, sqrt, arctan, sinh, cosh, tanh = (np.frompyfunc(f, 1, 1) for f in (mp.cos, mp.sin, mp.sqrt, mp.atan, mp.sinh, mp.cosh, mp.tanh))
    arctan2 = np.frompyfunc(mp.atan2, 2, 1)


def split(t):
    hi = np.frompyfunc(float, 1, 1)(t).astype(np.float64)
    lo = np.frompyfunc(lambda v, h: float(v - mp.mpf(float(h))), 2, 1)(t, hi).astype(np.float64)
    return np.stack([hi, lo])


def table():
    out = {"dps": np.array(mp.mp.dps), "cases": np.array([c[0] for c in rd.CASES]), "fields": np.array(rd.FIELDS)}
    eref = np.zeros((len(rd.CASES), len(rd.FIELDS)))
    for k, case in enumerate(rd.CASES):
        truth = rd.regional(M=MP, **rd.case_args(case))
        fp64 = rd.regional(**rd.case_args(case))
        for f, name in enumerate(rd.FIELDS):
            t = split(truth[name])
            out["%s/%s" % (case[0], name)] = t
            eref[k, f] = rd.error(name, fp64[name], t[0], t[1]).max()
        print("%-20s %s" % (case[0], " ".join("%s %.2e" % (n, e) for n, e in zip(rd.FIELDS, eref[k]))))
    out["eref"] = eref
    return out


def main():
    out = table()
    np.savez_compressed(OUT, **out)
    print("%d cases, %d points; wrote %s, %d bytes" % (len(rd.CASES), sum(out[c[0] + "/x"][0].size for c in rd.CASES), OUT,
                                                        os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
