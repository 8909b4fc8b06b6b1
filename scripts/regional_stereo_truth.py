#!/usr/bin/env python3
"""Extended-precision TRUTH for the stereographic regional grids on the cases of tests/regional_stereo_definition.py (CASES).

CPU only (mpmath, 50 digits):

    python scripts/regional_stereo_truth.py      ->  tests/golden/regional_stereo_truth.npz

As scripts/regional_truth.py: the statements of the definition (include/ogg_hip.h, "Stereographic regional grids";
tests/regional_stereo_definition.py) on the same fp64 arguments, with every operation and every transcendental carried to 50 digits, pi
included, and rounded once at the end.  |fp64 definition - truth| is the definition's own rounding error, the yardstick the device is
held to (tests/test_gpu_regional_stereo.py).

Stored: ``cases`` (the names, in the order of CASES); per case and field "<case>/<field>" the truth of the whole grid as an array
(2, rows, columns): hi = fp64(truth) and lo = fp64(truth - hi); and ``eref`` (cases x fields, the order of FIELDS): the fp64
definition's largest distance from the truth as measured when the file was made, in degrees for x, y, angle_dx and relative to the
truth for dx, dy, area.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, HERE)
import regional_stereo_definition as sd  # noqa: E402
from regional_truth import MP, mp, split  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "regional_stereo_truth.npz")


def table():
    out = {"dps": np.array(mp.mp.dps), "cases": np.array([c[0] for c in sd.CASES]), "fields": np.array(sd.FIELDS)}
    eref = np.zeros((len(sd.CASES), len(sd.FIELDS)))
    for k, case in enumerate(sd.CASES):
        truth = sd.stereo(M=MP, **sd.case_args(case))
        fp64 = sd.stereo(**sd.case_args(case))
        for f, name in enumerate(sd.FIELDS):
            t = split(truth[name])
            out["%s/%s" % (case[0], name)] = t
            eref[k, f] = sd.error(name, fp64[name], t[0], t[1]).max()
        print("%-20s %s" % (case[0], " ".join("%s %.2e" % (n, e) for n, e in zip(sd.FIELDS, eref[k]))))
    out["eref"] = eref
    return out


def main():
    out = table()
    np.savez_compressed(OUT, **out)
    print("%d cases, %d points; wrote %s, %d bytes" % (len(sd.CASES), sum(out[c[0] + "/x"][0].size for c in sd.CASES), OUT,
                                                        os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
