"""The polar stereographic projection of include/ogg_hip.h ("Layered topography") at 50 digits: tests/golden/stereo_truth.npz.

    python scripts/stereo_truth.py [-o tests/golden/stereo_truth.npz]

Eight cases (both hemispheres; the WGS84 ellipsoid and the sphere e = 0; lat_ts of 70, -71, -65 and the pole itself; lon0 of 0, -45 and
170) of 500 points each: latitudes from 40 degrees from the equator to within 1e-9 degrees of the pole (dense towards the pole), longitudes
over two turns, and clusters within 1e-3 .. 1e-12 degrees of lon - lon0 = 0, +-90 and 180, where a coordinate passes through zero.
The inputs are the fp64 numbers lon, lat, lat_ts, lon0, a and e taken as exact; everything else (pi, K) is formed at 50 digits.  X and Y
are stored as an fp64 head and tail (X = X_hi + X_lo to about 32 digits): a coordinate of 4e6 m has an ulp of 9e-10 m, which is the size
of the errors to be measured.  Needs mpmath; the tests read only the file.
"""
import argparse
import os

import mpmath as mp
import numpy as np

mp.mp.dps = 50
A_WGS84, RF_WGS84 = 6378137.0, 298.257223563
E_WGS84 = float(np.sqrt(2.0 / RF_WGS84 - 1.0 / RF_WGS84 ** 2))
# h, lat_ts, lon0, a, e
CASES = ((-1, -71.0, 0.0, A_WGS84, E_WGS84), (1, 70.0, -45.0, A_WGS84, E_WGS84), (-1, -65.0, 170.0, A_WGS84, E_WGS84),
         (1, 90.0, 0.0, A_WGS84, E_WGS84), (-1, -90.0, -45.0, A_WGS84, E_WGS84), (-1, -71.0, 0.0, A_WGS84, 0.0),
         (1, 70.0, -45.0, 6371000.0, 0.0), (1, 90.0, 170.0, 6371000.0, 0.0))
N_POINTS = 500


def t_of(e, phi):
    s, c = mp.sin(phi), mp.cos(phi)
    return c / (1 + s) * mp.exp(e * mp.atanh(e * s))


def project(h, lat_ts, lon0, a, e, lon, lat):
    """(X, Y) of one point, every argument an exact fp64 number, in mpmath"""
    h, lat_ts, lon0, a, e, lon, lat = (mp.mpf(v) for v in (h, lat_ts, lon0, a, e, lon, lat))
    rad = mp.pi / 180
    phi_ts = h * lat_ts * rad
    if h * lat_ts == 90:
        K = 2 * a / mp.sqrt((1 + e) ** (1 + e) * (1 - e) ** (1 - e))
    else:
        K = a * (mp.cos(phi_ts) / mp.sqrt(1 - e * e * mp.sin(phi_ts) ** 2)) / t_of(e, phi_ts)
    rho = K * t_of(e, h * lat * rad)
    lam = h * (lon - lon0) * rad
    return h * rho * mp.sin(lam), -h * rho * mp.cos(lam)


def points(case, rng):
    """lon, lat (fp64) of one case"""
    h, _, lon0, _, _ = case
    n_log, n_uni, n_cluster = 300, 100, 100
    colat = np.concatenate([10.0 ** rng.uniform(-9.0, np.log10(50.0), n_log), rng.uniform(0.0, 50.0, n_uni),
                            10.0 ** rng.uniform(-9.0, np.log10(50.0), n_cluster)])
    colat[0], colat[1] = 1.0e-9, 50.0
    lat = h * (90.0 - colat)
    lon = rng.uniform(-360.0, 360.0, n_log + n_uni + n_cluster)
    k = np.arange(n_cluster)
    off = np.where(k % 3 == 0, 0.0, rng.choice([-1.0, 1.0], n_cluster) * 10.0 ** rng.uniform(-12.0, -3.0, n_cluster))
    lon[n_log + n_uni:] = lon0 + np.array([0.0, 90.0, -90.0, 180.0])[k % 4] + off + 360.0 * rng.integers(-1, 2, n_cluster)
    return lon, lat


def head_tail(v):
    hi = float(v)
    return hi, float(v - mp.mpf(hi))


def main(argv=None):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("-o", "--output", default=os.path.join(root, "tests", "golden", "stereo_truth.npz"))
    a = p.parse_args(argv)
    rng = np.random.default_rng(20261020)
    n = len(CASES) * N_POINTS
    out = {k: np.zeros(n) for k in ("lon", "lat", "X_hi", "X_lo", "Y_hi", "Y_lo")}
    out["case"] = np.repeat(np.arange(len(CASES)), N_POINTS).astype(np.int32)
    for ci, case in enumerate(CASES):
        lon, lat = points(case, rng)
        sl = slice(ci * N_POINTS, (ci + 1) * N_POINTS)
        out["lon"][sl], out["lat"][sl] = lon, lat
        for k in range(N_POINTS):
            X, Y = project(*case, lon[k], lat[k])
            i = ci * N_POINTS + k
            out["X_hi"][i], out["X_lo"][i] = head_tail(X)
            out["Y_hi"][i], out["Y_lo"][i] = head_tail(Y)
    np.savez_compressed(a.output, cases=np.array(CASES, dtype=np.float64), **out)
    print("%s: %d points of %d cases" % (a.output, n, len(CASES)))


if __name__ == "__main__":
    main()
