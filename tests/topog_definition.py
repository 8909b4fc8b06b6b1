"""The numpy definition of topography by refined sampling (include/ogg_hip.h, "Topography by refined sampling"), restated operation
for operation, used by tests/test_topog_cpu.py and tests/test_gpu_topog.py.  Slow (every sample is materialised), so for small
grids only."""
import numpy as np

MAX_R = 256
POLE_EPS = 1.0e-10
MISSING = np.iinfo(np.int32).min
RECORD_FIELDS = ("n", "n_missing", "n_wet", "sum", "sumsq", "min", "max", "R", "n_pole", "n_clamped")


def quantise(raw, quantum=None, fill=()):
    """(q as int32 with MISSING where the raw value is missing, quantum): int16 as it is, floats rint(v / quantum) in fp64."""
    raw = np.asarray(raw)
    v = raw.astype(np.float64)
    missing = np.isnan(v)
    for f in fill:
        missing |= v == float(raw.dtype.type(f))
    if raw.dtype == np.int16:
        q = raw.astype(np.int32)
        quantum = 1.0 if quantum is None else float(quantum)
    else:
        quantum = 0.01 if quantum is None else float(quantum)
        with np.errstate(invalid="ignore"):
            r = np.rint(v / quantum)
        if np.any(np.abs(r[~missing]) > 2 ** 21):
            raise ValueError("a quantised value exceeds 2^21")
        q = np.where(missing, 0.0, r).astype(np.int32)
    return np.where(missing, MISSING, q).astype(np.int32), quantum


def _wrap(d):
    return (d + 180.0) % 360.0 - 180.0


def cells(x, y, dlon, dlat, refine=None, oversample=2.0):
    """Per supergrid cell: L00, L01, L10, L11, y00, y01, y10, y11, R, clamped, pole (0, -1 south, +1 north)."""
    x00, x01, x10, x11 = x[:-1, :-1], x[:-1, 1:], x[1:, :-1], x[1:, 1:]
    y00, y01, y10, y11 = y[:-1, :-1], y[:-1, 1:], y[1:, :-1], y[1:, 1:]
    l00, l01, l10, l11 = (x00 + _wrap(v - x00) for v in (x00, x01, x10, x11))
    pl = 90.0 - POLE_EPS
    L00 = np.where(np.abs(y00) >= pl, l01, l00)
    L01 = np.where(np.abs(y01) >= pl, l00, l01)
    L10 = np.where(np.abs(y10) >= pl, l11, l10)
    L11 = np.where(np.abs(y11) >= pl, l10, l11)
    if refine:
        R = np.full(x00.shape, int(refine), dtype=np.int64)
        clamped = np.zeros(x00.shape, dtype=bool)
    else:
        Ls, Ys = np.stack([L00, L01, L10, L11]), np.stack([y00, y01, y10, y11])
        span_l = Ls.max(axis=0) - Ls.min(axis=0)
        span_y = Ys.max(axis=0) - Ys.min(axis=0)
        v = np.ceil(oversample * np.maximum(span_l / dlon, span_y / dlat))
        clamped = ~(v <= MAX_R)
        R = np.where(clamped, MAX_R, np.where(v < 1.0, 1.0, v)).astype(np.int64)
    w = _wrap(L01 - L00) + _wrap(L11 - L01) + _wrap(L10 - L11) + _wrap(L00 - L10)
    north = (y00 + y01 + y10 + y11) > 0.0
    pole = np.where(np.abs(w) > 180.0, np.where(north, 1, -1), 0)
    return dict(L00=L00, L01=L01, L10=L10, L11=L11, y00=y00, y01=y01, y10=y10, y11=y11, R=R, clamped=clamped, pole=pole)


def sample_positions(c, R, idx):
    """lon, lat (cells x R x R, [cell, b, a]) of the cells idx (all of refinement R); a pole cell's lat is not used."""
    k = np.arange(R)
    S = (k + 0.5) / R
    U = 1.0 - S
    sa, ua = S[None, None, :], U[None, None, :]
    tb, vb = S[None, :, None], U[None, :, None]
    w00, w01, w10, w11 = ua * vb, sa * vb, ua * tb, sa * tb
    g = {k_: c[k_][idx][:, None, None] for k_ in ("L00", "L01", "L10", "L11", "y00", "y01", "y10", "y11")}
    lon = w00 * g["L00"] + w01 * g["L01"] + w10 * g["L10"] + w11 * g["L11"]
    lat = w00 * g["y00"] + w01 * g["y01"] + w10 * g["y10"] + w11 * g["y11"]
    pole = c["pole"][idx] != 0
    if np.any(pole):
        lon = np.where(pole[:, None, None], g["L00"] + 360.0 * sa, lon)
    return lon, lat


def sample_values(q, lon0, dlon, lat0, dlat, lon, lat, pole):
    """(value, missing) of every sample; pole: per cell 0 / -1 / +1."""
    Ny, Nx = q.shape
    periodic = abs(Nx * dlon - 360.0) <= 1e-9
    inv_dlon, inv_dlat = 1.0 / dlon, 1.0 / dlat
    pj = pole[:, None, None]
    miss = np.zeros(lon.shape, dtype=bool)
    with np.errstate(invalid="ignore", over="ignore"):
        fj = np.floor((lat - lat0) * inv_dlat)
        if periodic:
            fi = np.floor((lon - lon0) * inv_dlon)
            miss |= ~(np.abs(fi) < 4.0e15)            # a longitude that is not finite (or beyond any grid): no index is formed
            is_ = np.where(miss, 0.0, fi).astype(np.int64) % Nx
            finite = np.abs(fj) < np.inf
            miss |= (pj == 0) & ~finite                # a latitude that is not finite is MISSING, not clamped
            fj = np.clip(np.where(finite, fj, 0.0), 0.0, Ny - 1.0)
        else:
            d = (lon - lon0) % 360.0                   # onto the raster's own branch; d itself when 0 <= d < 360 (fmod is exact)
            fi = np.floor(d * inv_dlon)
            miss |= ~((fi >= 0) & (fi < Nx))
            is_ = np.where(miss, 0.0, fi).astype(np.int64)
            miss |= (pj == 0) & ~((fj >= 0) & (fj < Ny))
    js = np.where(pj < 0, 0, np.where(pj > 0, Ny - 1, np.where(miss, 0, fj))).astype(np.int64)   # a pole cell: the polar row
    v = q[js, np.where(miss, 0, is_)]
    miss |= v == MISSING
    return v, miss


def supergrid_records(x, y, q, lon0, dlon, lat0, dlat, refine=None, oversample=2.0, wet_below=0.0):
    """Records of every supergrid cell (a dict of arrays ny x nx, RECORD_FIELDS)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    with np.errstate(invalid="ignore"):   # a grid point that is not finite
        c = cells(x, y, dlon, dlat, refine, oversample)
    shape = c["R"].shape
    out = {f: np.zeros(shape, dtype=np.int64) for f in RECORD_FIELDS}
    out["min"][:] = np.iinfo(np.int32).max
    out["max"][:] = np.iinfo(np.int32).min
    out["R"] = c["R"].copy()
    out["n_pole"] = (c["pole"] != 0).astype(np.int64)
    out["n_clamped"] = c["clamped"].astype(np.int64)
    flatR = c["R"].reshape(-1)
    flat = {k: v.reshape(-1) for k, v in c.items()}
    for R in np.unique(flatR):
        all_idx = np.nonzero(flatR == R)[0]
        chunk = max(1, 4_000_000 // int(R * R))
        for s0 in range(0, all_idx.size, chunk):
            idx = all_idx[s0:s0 + chunk]
            with np.errstate(invalid="ignore"):
                lon, lat = sample_positions(flat, int(R), idx)
            v, miss = sample_values(q, lon0, dlon, lat0, dlat, lon, lat, flat["pole"][idx])
            ok = ~miss
            v64 = v.astype(np.int64)
            o = {k: out[k].reshape(-1) for k in out}
            o["n"][idx] = ok.sum(axis=(1, 2))
            o["n_missing"][idx] = miss.sum(axis=(1, 2))
            o["n_wet"][idx] = (ok & (v.astype(np.float64) < wet_below)).sum(axis=(1, 2))
            o["sum"][idx] = np.where(ok, v64, 0).sum(axis=(1, 2))
            o["sumsq"][idx] = np.where(ok, v64 * v64, 0).sum(axis=(1, 2))
            o["min"][idx] = np.where(ok, v64, np.iinfo(np.int32).max).min(axis=(1, 2))
            o["max"][idx] = np.where(ok, v64, np.iinfo(np.int32).min).max(axis=(1, 2))
    return out


def model_records(sg):
    """2 x 2 blocks of supergrid records."""
    out = {}
    for f in RECORD_FIELDS:
        a = sg[f]
        blocks = [a[0::2, 0::2], a[0::2, 1::2], a[1::2, 0::2], a[1::2, 1::2]]
        if f == "min":
            out[f] = np.minimum.reduce(blocks)
        elif f in ("max", "R"):
            out[f] = np.maximum.reduce(blocks)
        else:
            out[f] = blocks[0] + blocks[1] + blocks[2] + blocks[3]
    return out


def records(x, y, raw, lon0, dlon, lat0, dlat, refine=None, oversample=2.0, quantum=None, sea_level=0.0, cells_="model", fill=()):
    q, quantum = quantise(raw, quantum, fill)
    sg = supergrid_records(x, y, q, lon0, dlon, lat0, dlat, refine, oversample, float(sea_level) / quantum)
    return model_records(sg) if cells_ == "model" else sg


def samples_per_second_baseline(x, y, raw, box, repeat=1):
    """Host samples/s of this definition on one core (the baseline the device is compared with)."""
    import time
    q, _ = quantise(raw)
    t0 = time.perf_counter()
    for _ in range(repeat):
        r = supergrid_records(x, y, q, *box)
    dt = (time.perf_counter() - t0) / repeat
    return float((r["n"] + r["n_missing"]).sum()) / dt
