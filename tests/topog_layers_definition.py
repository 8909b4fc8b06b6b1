"""The numpy definition of layered topography (include/ogg_hip.h, "Layered topography"), restated operation for operation on top of
tests/topog_definition.py; used by tests/test_topog_layers_cpu.py and tests/test_gpu_topog_layers.py.  Slow (every sample is
materialised), so for small grids only.  Not part of the product package."""
import os

import numpy as np

import topog_definition as D

MAX_SOURCES = 4
LATLON, POLAR_STEREO = 0, 1
MAX_Q = 2 ** 21
PI_180 = np.pi / 180.0
RECORD_FIELDS = D.RECORD_FIELDS
TRUTH = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stereo_truth.npz")


def t_factor(e, phi):
    s, c = np.sin(phi), np.cos(phi)
    return c / (1.0 + s) * np.exp(e * np.arctanh(e * s))


def stereo_K(h, lat_ts, a, e):
    """K of the header: a * m_ts / t_ts, and its limit at the pole"""
    if h * lat_ts == 90.0:
        return 2.0 * a / np.sqrt((1.0 + e) ** (1.0 + e) * (1.0 - e) ** (1.0 - e))
    phi = h * lat_ts * PI_180
    return a * (np.cos(phi) / np.sqrt(1.0 - e * e * np.sin(phi) ** 2)) / t_factor(e, phi)


class Stereo(object):
    def __init__(self, h, lat_ts, lon0, a, e, lat_gate=-80.0):
        self.h, self.lat_ts, self.lon0, self.a, self.e, self.lat_gate = int(h), float(lat_ts), float(lon0), float(a), float(e), float(lat_gate)
        self.K = float(stereo_K(self.h, self.lat_ts, self.a, self.e))


def project(p, lon, lat):
    """X, Y, ok of the header's projection (ok: finite and through the gate; X = Y = 0 where not)"""
    lon, lat = np.broadcast_arrays(np.asarray(lon, dtype=np.float64), np.asarray(lat, dtype=np.float64))
    h = float(p.h)
    with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
        hl = h * lat
        ok = (np.abs(lon) < np.inf) & (np.abs(lat) < np.inf) & (hl >= p.lat_gate)
        lon_, hl_ = np.where(ok, lon, p.lon0), np.where(ok, hl, 0.0)
        phi, lam = hl_ * PI_180, h * (lon_ - p.lon0) * PI_180
        s, c = np.sin(phi), np.cos(phi)
        rho = (p.K * c) / (1.0 + s) * np.exp(p.e * np.arctanh(p.e * s))
        X, Y = h * (rho * np.sin(lam)), -h * (rho * np.cos(lam))
    polar = hl_ >= 90.0 - D.POLE_EPS
    X, Y = np.where(ok & ~polar, X, 0.0), np.where(ok & ~polar, Y, 0.0)
    return X, Y, ok


def layer(raw, box, proj=None, q_mul=1, quantum=None, fill=()):
    """A layer: the raster quantised as topog_definition does, its box (lon0, dlon, lat0, dlat or X0, dX, Y0, dY) and projection"""
    q, quantum = D.quantise(raw, quantum, fill)
    bad = (q != D.MISSING) & (np.abs(q.astype(np.int64) * int(q_mul)) > MAX_Q)
    if np.any(bad):
        raise ValueError("q_mul times a stored value exceeds 2^21")
    return dict(q=q, box=tuple(float(v) for v in box), proj=proj, q_mul=int(q_mul), quantum=quantum,
                kind=LATLON if proj is None else POLAR_STEREO, raw=np.asarray(raw), fill=tuple(fill))


def fractional_index(ly, lon, lat, pole):
    """(fx, fy, ok) of samples in a projected layer: the unfloored indices and whether the sample is projected at all"""
    pj = pole[:, None, None]
    X, Y, ok = project(ly["proj"], lon, np.where(pj != 0, 90.0 * pj, lat))
    X0, dX, Y0, dY = ly["box"]
    return (X - X0) * (1.0 / dX), (Y - Y0) * (1.0 / dY), ok


def layer_values(ly, lon, lat, pole):
    """(value times q_mul, missing) of every sample in one layer"""
    q = ly["q"]
    if ly["kind"] == LATLON:
        v, miss = D.sample_values(q, *ly["box"], lon, lat, pole)
    else:
        Ny, Nx = q.shape
        fx, fy, ok = fractional_index(ly, lon, lat, pole)
        fi, fj = np.floor(fx), np.floor(fy)
        miss = ~(ok & (fi >= 0) & (fi < Nx) & (fj >= 0) & (fj < Ny))
        v = q[np.where(miss, 0, fj).astype(np.int64), np.where(miss, 0, fi).astype(np.int64)]
        miss = miss | (v == D.MISSING)
    return np.where(miss, 0, v.astype(np.int64) * ly["q_mul"]), miss


def refinement(x, y, layers, refine=None, oversample=2.0):
    """The cells of topog_definition.cells with the header's R over the layers"""
    c = D.cells(x, y, 1.0, 1.0, refine=1)
    shape = c["R"].shape
    if refine:
        c["R"] = np.full(shape, int(refine), dtype=np.int64)
        return c
    clamped, R = np.zeros(shape, dtype=bool), np.ones(shape, dtype=np.int64)
    Ls, Ys = np.stack([c[k] for k in ("L00", "L01", "L10", "L11")]), np.stack([c[k] for k in ("y00", "y01", "y10", "y11")])
    for ly in layers:
        if ly["kind"] == LATLON:
            ck = D.cells(x, y, ly["box"][1], ly["box"][3], None, oversample)
            clamped |= ck["clamped"]
            R = np.maximum(R, ck["R"])
            continue
        X0, dX, Y0, dY = ly["box"]
        Ny, Nx = ly["q"].shape
        X, Y, ok = project(ly["proj"], Ls, Ys)
        fi, fj = np.floor((X - X0) * (1.0 / dX)), np.floor((Y - Y0) * (1.0 / dY))
        inside = ok & (fi >= 0) & (fi < Nx) & (fj >= 0) & (fj < Ny)
        span = lambda v: np.where(ok, v, -np.inf).max(axis=0) - np.where(ok, v, np.inf).min(axis=0)   # noqa: E731
        with np.errstate(invalid="ignore"):
            v = np.where(inside.any(axis=0), np.ceil(oversample * np.maximum(span(X) / dX, span(Y) / dY)), 1.0)
        clamped |= ~(v <= D.MAX_R)
        R = np.maximum(R, np.where(v <= D.MAX_R, np.maximum(v, 1.0), 1.0).astype(np.int64))
    c["clamped"], c["R"] = clamped, np.where(clamped, D.MAX_R, R)
    return c


def supergrid_records(x, y, layers, refine=None, oversample=2.0, wet_below=0.0, with_edge=False):
    """Merge records of every supergrid cell: RECORD_FIELDS (ny x nx) and n_from (4 x ny x nx).  ``with_edge``: also "edge", per cell
    the smallest distance of a projected sample's fractional index (either axis, any projected layer) from an integer (inf: none)"""
    if not 1 <= len(layers) <= MAX_SOURCES:
        raise ValueError("1 .. %d layers" % MAX_SOURCES)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        c = refinement(x, y, layers, refine, oversample)
    shape = c["R"].shape
    out = {f: np.zeros(shape, dtype=np.int64) for f in RECORD_FIELDS}
    out["min"][:] = np.iinfo(np.int32).max
    out["max"][:] = np.iinfo(np.int32).min
    out["R"] = c["R"].copy()
    out["n_pole"] = (c["pole"] != 0).astype(np.int64)
    out["n_clamped"] = c["clamped"].astype(np.int64)
    n_from = np.zeros((MAX_SOURCES, shape[0] * shape[1]), dtype=np.int64)
    edge = np.full(shape[0] * shape[1], np.inf)
    flatR = c["R"].reshape(-1)
    flat = {k: v.reshape(-1) for k, v in c.items()}
    o = {k: out[k].reshape(-1) for k in out}
    for R in np.unique(flatR):
        all_idx = np.nonzero(flatR == R)[0]
        chunk = max(1, 2_000_000 // int(R * R))
        for s0 in range(0, all_idx.size, chunk):
            idx = all_idx[s0:s0 + chunk]
            with np.errstate(invalid="ignore"):
                lon, lat = D.sample_positions(flat, int(R), idx)
            pole = flat["pole"][idx]
            miss = np.ones(lon.shape, dtype=bool)
            v = np.zeros(lon.shape, dtype=np.int64)
            for k, ly in enumerate(layers):
                vk, mk = layer_values(ly, lon, lat, pole)
                take = miss & ~mk
                v = np.where(take, vk, v)
                n_from[k, idx] = take.sum(axis=(1, 2))
                miss &= mk
                if with_edge and ly["kind"] == POLAR_STEREO:
                    fx, fy, okp = fractional_index(ly, lon, lat, pole)
                    d = np.minimum(np.abs(fx - np.rint(fx)), np.abs(fy - np.rint(fy)))
                    edge[idx] = np.minimum(edge[idx], np.where(okp, d, np.inf).min(axis=(1, 2)))
            ok = ~miss
            o["n"][idx] = ok.sum(axis=(1, 2))
            o["n_missing"][idx] = miss.sum(axis=(1, 2))
            o["n_wet"][idx] = (ok & (v.astype(np.float64) < wet_below)).sum(axis=(1, 2))
            o["sum"][idx] = np.where(ok, v, 0).sum(axis=(1, 2))
            o["sumsq"][idx] = np.where(ok, v * v, 0).sum(axis=(1, 2))
            o["min"][idx] = np.where(ok, v, np.iinfo(np.int32).max).min(axis=(1, 2))
            o["max"][idx] = np.where(ok, v, np.iinfo(np.int32).min).max(axis=(1, 2))
    out["n_from"] = n_from.reshape((MAX_SOURCES,) + shape)
    if with_edge:
        out["edge"] = edge.reshape(shape)
    return out


def model_records(sg):
    """2 x 2 blocks of supergrid merge records (n_from adds; edge: the smallest)"""
    out = D.model_records(sg)
    a = sg["n_from"]
    out["n_from"] = a[:, 0::2, 0::2] + a[:, 0::2, 1::2] + a[:, 1::2, 0::2] + a[:, 1::2, 1::2]
    if "edge" in sg:
        e = sg["edge"]
        out["edge"] = np.minimum.reduce([e[0::2, 0::2], e[0::2, 1::2], e[1::2, 0::2], e[1::2, 1::2]])
    return out


def records(x, y, layers, refine=None, oversample=2.0, sea_level=0.0, cells_="model", with_edge=False):
    """The list's quantum is that of the layer with q_mul = 1 (layers[k].quantum / q_mul, the same for every k)"""
    quantum = layers[0]["quantum"] / layers[0]["q_mul"]
    sg = supergrid_records(x, y, layers, refine, oversample, float(sea_level) / quantum, with_edge)
    return model_records(sg) if cells_ == "model" else sg


# ---- the truth file ------------------------------------------------------------------------------------------------
def truth_cases():
    """[(Stereo, lon, lat, X_hi, X_lo, Y_hi, Y_lo)] of tests/golden/stereo_truth.npz (scripts/stereo_truth.py), gate at 35 degrees"""
    z = np.load(TRUTH)
    out = []
    for ci, (h, lat_ts, lon0, a, e) in enumerate(z["cases"]):
        m = z["case"] == ci
        out.append((Stereo(int(h), lat_ts, lon0, a, e, lat_gate=35.0),) + tuple(z[k][m] for k in ("lon", "lat", "X_hi", "X_lo", "Y_hi", "Y_lo")))
    return out


def truth_errors(X, Y, case):
    """(error in metres, error relative to rho) of every point of one truth case: the distance from the truth in the plane"""
    _, _, _, xh, xl, yh, yl = case
    err = np.hypot((X - xh) - xl, (Y - yh) - yl)
    return err, err / np.hypot(xh, yh)


def definition_error():
    """E_def: the largest error of project() over the truth file, (metres, relative to rho)"""
    em, er = 0.0, 0.0
    for case in truth_cases():
        X, Y, ok = project(case[0], case[1], case[2])
        assert ok.all()
        m, r = truth_errors(X, Y, case)
        em, er = max(em, float(m.max())), max(er, float(r.max()))
    return em, er
