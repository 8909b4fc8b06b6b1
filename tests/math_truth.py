"""Extended-precision truth, argument generators and numpy restatements for the range-specialised device helpers (csrc/ogg_math.h,
ogg_bipolar_dev.h, ogg_dpole_dev.h) that tests/test_gpu_math_helpers.py evaluates through ogg_math_eval_dev.  A plain module: no
fixtures, no GPU.  tests/test_math_truth_cpu.py checks this module itself.

Truth.  ``truth(name, x, y, path)`` returns the exact function of the fp64 arguments as hi + lo doubles (hi the fp64 value nearest
the truth) on one of two paths:
  * "longdouble": numpy.longdouble through the C library's long-double functions, where its eps is at most 2^-63 (x87: 2^-63); the
    truth is then good to about one long-double ulp, 2^-10 of an fp64 ulp;
  * "mpmath": mpmath at 50 digits, exact for every purpose here, ~30 us per argument.
``measure`` takes a device result's error in ulps of hi on the long-double path and RE-MEASURES with mpmath every argument whose error
lies within 2^-8 ulp of the worst one (four times the long-double truth's own error, so the true worst case is among them): the
reported maximum has mpmath's precision, at long-double cost.  Without an 80-bit long double the bulk is a subsample of at least
20 000 arguments, every one through mpmath, the edge arguments always among them.  ``PATH`` says which of the two this machine takes.
"""
import numpy as np

LD = np.longdouble
LONGDOUBLE_OK = bool(np.finfo(LD).eps <= 2.0 ** -63)
PATH = "longdouble+mpmath-refined" if LONGDOUBLE_OK else "mpmath-subsample"
MP_DIGITS = 50
MP_SUBSAMPLE = 20000
REFINE_WINDOW_ULP = 2.0 ** -8

PI_180 = np.pi / 180
TAN_PI_8 = 0.41421356237309503          # the literal of atan2_angle
HALF_PI = 1.5707963267948966
PIO2_1 = 1.57079632673412561417e+00     # cos_cap: the 33-bit head of pi/2
COS_CAP_LO, COS_CAP_HI = -2.356194490192345, -0.7853981633974483   # cos_cap: x in (LO, HI) ...
COS_CAP_GAP = 2.0 ** -20                # ... and |x + PIO2_1| >= GAP
TINY_LIMIT = 2.0 ** -13                 # sin_tiny / asin_tiny: |x| < TINY_LIMIT
ATAN_CAP_LIMIT = 0.3                    # atan_cap: u <= 0.3
ARC_SWITCH = 1e-3                       # homogeneous_arc: series below, atan_lib at or above

# ---------------------------------------------------------------------------------------------------------------
# truth
# ---------------------------------------------------------------------------------------------------------------
_LD_FUNCS = {
    "rcp": lambda x, y: LD(1) / x,
    "rsqrt": lambda x, y: LD(1) / np.sqrt(x),
    "atan": lambda x, y: np.arctan(x),
    "atan2": lambda x, y: np.where((x == 0) & (y == 0), np.copysign(LD(0), y), np.arctan2(y, x)),   # atan2_angle's own convention at the origin: 0
    "sin": lambda x, y: np.sin(x),
    "asin": lambda x, y: np.arcsin(x),
    "cos": lambda x, y: np.cos(x),
}
NAMES = tuple(sorted(_LD_FUNCS))


def _mp_func(name):
    import mpmath as mp
    return {"rcp": lambda x, y: 1 / x, "rsqrt": lambda x, y: 1 / mp.sqrt(x), "atan": lambda x, y: mp.atan(x),
            "atan2": lambda x, y: mp.atan2(y, x) if (x != 0 or y != 0) else mp.mpf(0), "sin": lambda x, y: mp.sin(x),
            "asin": lambda x, y: mp.asin(x), "cos": lambda x, y: mp.cos(x)}[name]


def truth_longdouble(name, x, y=None):
    """hi, lo (fp64 arrays) with hi + lo the long-double value of the function"""
    assert LONGDOUBLE_OK
    x = np.asarray(x, dtype=np.float64)
    with np.errstate(all="ignore"):
        t = _LD_FUNCS[name](x.astype(LD), None if y is None else np.asarray(y, dtype=np.float64).astype(LD))
        hi = t.astype(np.float64)
        lo = (t - hi.astype(LD)).astype(np.float64)
    return hi, lo


def truth_mpmath(name, x, y=None):
    """hi, lo (fp64 arrays) with hi + lo the 50-digit value of the function"""
    import mpmath as mp
    x = np.asarray(x, dtype=np.float64)
    f = _mp_func(name)
    hi, lo = np.empty(x.shape), np.empty(x.shape)
    ys = np.zeros(x.shape) if y is None else np.asarray(y, dtype=np.float64)
    with mp.workdps(MP_DIGITS):
        for k in range(x.size):
            t = f(mp.mpf(float(x.flat[k])), mp.mpf(float(ys.flat[k])))
            if name == "atan2" and ys.flat[k] == 0 and np.signbit(ys.flat[k]):
                t = -t   # mpmath has one zero: atan2(-0.0, x < 0) is -pi
            h = float(t)
            if h == 0.0:   # mpmath has one zero; the odd functions (and atan2 in y) keep the sign of theirs
                h = float(np.copysign(0.0, ys.flat[k] if name == "atan2" else x.flat[k]))
            hi.flat[k], lo.flat[k] = h, float(t - mp.mpf(h))
    return hi, lo


def truth(name, x, y=None, path=None):
    if path is None:
        path = "longdouble" if LONGDOUBLE_OK else "mpmath"
    return truth_longdouble(name, x, y) if path == "longdouble" else truth_mpmath(name, x, y)


def ulp_of(hi):
    """the fp64 ulp at the value nearest the truth"""
    return np.spacing(np.abs(hi))


def abs_errors_of(v, hi, lo):
    """|v - (hi + lo)| as fp64 (formed in long double where there is one; v - hi is exact for any v within a factor 2 of hi)"""
    if LONGDOUBLE_OK:
        return np.abs((v.astype(LD) - hi.astype(LD)) - lo.astype(LD)).astype(np.float64)
    return np.abs((v - hi) - lo)


def measure(name, v, x, y=None, keep=None, relative_to="ulp"):
    """Errors of the device values v = helper(x[, y]) against the truth ``name``.  Returns (idx, err): the arguments measured -- all of
    them on the long-double path, a subsample of >= MP_SUBSAMPLE that contains the indices ``keep`` otherwise -- and their errors, in
    ulps of the fp64 value nearest the truth (relative_to="ulp"), as |error / truth| ("rel") or absolute ("abs").  On the long-double
    path every argument within REFINE_WINDOW_ULP (or the same share of the worst error) of the worst is re-measured with mpmath."""
    v, x = np.asarray(v, dtype=np.float64), np.asarray(x, dtype=np.float64)
    y = None if y is None else np.asarray(y, dtype=np.float64)

    def scaled(e, hi):
        with np.errstate(all="ignore"):
            if relative_to == "ulp":
                return e / ulp_of(hi)
            if relative_to == "rel":
                return np.where(hi != 0.0, e / np.abs(hi), np.where(e == 0.0, 0.0, np.inf))
            return e

    if LONGDOUBLE_OK:
        idx = np.arange(x.size)
        hi, lo = truth_longdouble(name, x, y)
        err = scaled(abs_errors_of(v, hi, lo), hi)
        assert not np.isnan(err).any(), "NaN among the errors of %s" % name
        worst = err.max()
        window = REFINE_WINDOW_ULP if relative_to == "ulp" else worst * 2.0 ** -8
        again = np.nonzero(err >= worst - window)[0]
        if again.size > MP_SUBSAMPLE:   # a plateau (every error the same): the largest of them
            again = again[np.argsort(err[again])[-MP_SUBSAMPLE:]]
        hi2, lo2 = truth_mpmath(name, x[again], None if y is None else y[again])
        err[again] = scaled(abs_errors_of(v[again], hi2, lo2), hi2)
        return idx, err
    rng = np.random.RandomState(1)
    idx = np.arange(x.size) if x.size <= MP_SUBSAMPLE else rng.choice(x.size, MP_SUBSAMPLE, replace=False)
    if keep is not None:
        idx = np.union1d(idx, np.asarray(keep, dtype=np.int64))
    hi, lo = truth_mpmath(name, x[idx], None if y is None else y[idx])
    err = scaled(abs_errors_of(v[idx], hi, lo), hi)
    assert not np.isnan(err).any(), "NaN among the errors of %s" % name
    return idx, err


# ---------------------------------------------------------------------------------------------------------------
# arguments.  Every generator returns a dict of named fp64 arrays whose length is a multiple of 64 (whole waves: element k is lane
# k % 64 of wave k // 64) and deterministic; test_math_truth_cpu.py checks that every element lies in the domain the generator names.
# ---------------------------------------------------------------------------------------------------------------
def neighbours(v):
    v = np.float64(v)
    return [float(np.nextafter(v, -np.inf)), float(v), float(np.nextafter(v, np.inf))]


def spread(rng, n, e_lo, e_hi, signed=False):
    """n values m 2^e, m uniform in [1, 2), e uniform integer in [e_lo, e_hi): magnitudes in [2^e_lo, 2^e_hi)"""
    v = np.ldexp(1.0 + rng.random_sample(n), rng.randint(e_lo, e_hi, n))
    return v * (rng.randint(0, 2, n) * 2.0 - 1.0) if signed else v


def whole_waves(v, pad):
    """v padded with ``pad`` to a multiple of 64"""
    v = np.asarray(v, dtype=np.float64)
    r = (-v.size) % 64
    return np.concatenate([v, np.full(r, pad, dtype=np.float64)]) if r else v


def with_lane(v, lane, value):
    """a copy of v (whole waves) with ``value`` in lane ``lane`` of every wave: the "mixed" arrays"""
    w = np.array(v, dtype=np.float64)
    assert w.size % 64 == 0
    w[lane::64] = value
    return w


MIXED_LANE = 17


def div_pi180_args():
    rng = np.random.RandomState(21)
    m = np.array([1.0, 0.5, 3.0, 1e-300, 1e300, 2.0 ** -1000, 2.0 ** 1000 * (1 - 2.0 ** -53), np.pi, 1e-5, 7.0, 0.3, 1e10, 2.0 ** -500, 123.456,
                  2.0 ** 52, 1.0 + 2.0 ** -52, 2.0 ** -52, 90 * PI_180, 180 * PI_180, 45 * PI_180, 1e-17, 1e17, 6371e3, 2.5, 1e-100, 1e100,
                  0.1, 10.0, 1e-10, 65.0, 3e-7])
    tab = np.concatenate([[0.0, -0.0], m, -m])
    assert tab.size == 64
    with np.errstate(all="ignore"):
        at2 = np.arctan2(tab[:, None], tab[None, :]).ravel()
    return {"zeros": whole_waves([0.0, -0.0], 0.0),
            "binades": spread(rng, 1 << 20, -1000, 1000, signed=True),
            "radians": np.concatenate([np.linspace(-2 * np.pi, 2 * np.pi, 1 << 17), (rng.random_sample(1 << 17) * 4 - 2) * np.pi]),
            "arctan2_table": at2}


def rcp_rsqrt_args():
    rng = np.random.RandomState(22)
    p2 = np.ldexp(1.0, np.arange(-340, 341))
    edges = np.concatenate([np.nextafter(p2, 0)[1:], p2, np.nextafter(p2, np.inf)[:-1]])   # the powers of four and their neighbours among them
    return {"edges": whole_waves(edges, 1.0), "bulk": spread(rng, 1 << 19, -340, 340)}


def atan_cap_args():
    rng = np.random.RandomState(23)
    edges = [0.0, 2.0 ** -27, 5e-324, 2.2250738585072014e-308] + neighbours(ATAN_CAP_LIMIT)[:2] + neighbours(2.0 ** -27) + [0.23, 0.1, 1e-3]
    small = np.concatenate([spread(rng, 1 << 16, -1022, -2), rng.random_sample(1 << 12) * 2.0 ** -1022])   # below 0.25, down to the subnormals
    small = small[: small.size // 64 * 64]
    in_range = {"edges": whole_waves(edges, 0.3), "uniform": rng.random_sample(1 << 18) * ATAN_CAP_LIMIT, "log": small}
    above = np.concatenate([neighbours(ATAN_CAP_LIMIT)[2:], [0.31, 1.0, 1.5, 1e3, 1e300, np.inf, np.nan, 0.5]])
    base = rng.random_sample(64 * above.size) * ATAN_CAP_LIMIT
    mixed = base.copy()
    mixed[MIXED_LANE::64] = above            # one out-of-range lane per wave
    return in_range, {"mixed": mixed, "all_above": 0.3 + rng.random_sample(1 << 12) * 3 + 1e-9}


def atan2_angle_args():
    rng = np.random.RandomState(24)
    n = 1 << 18
    x, y = spread(rng, n, -300, 300, signed=True), spread(rng, n, -300, 300, signed=True)
    q = n // 2
    x[:q], y[:q] = rng.random_sample(q) * 4 - 2, rng.random_sample(q) * 4 - 2                     # comparable, in +-2
    k = 4096
    mag = spread(rng, k, -300, 300)
    sx, sy = rng.randint(0, 2, k) * 2.0 - 1.0, rng.randint(0, 2, k) * 2.0 - 1.0
    x[q:q + k], y[q:q + k] = sx * mag, sy * mag                                                   # |y| = |x|
    mxv = spread(rng, k, -290, 290)
    mnv = TAN_PI_8 * mxv                                                                          # next to mn = tan(pi/8) mx
    mnv = np.where(np.arange(k) % 3 == 0, np.nextafter(mnv, 0), np.where(np.arange(k) % 3 == 1, mnv, np.nextafter(mnv, np.inf)))
    swap = rng.randint(0, 2, k) == 1
    x[q + k:q + 2 * k], y[q + k:q + 2 * k] = sx * np.where(swap, mnv, mxv), sy * np.where(swap, mxv, mnv)
    x[q + 2 * k:q + 3 * k] = 0.0 * sx                                                             # x = +-0, y finite
    y[q + 3 * k:q + 4 * k] = 0.0 * sy                                                             # y = +-0, x finite
    fy = np.array([0.0, -0.0, 0.0, -0.0, 1.0, -1.0, 2.0 ** -300, -(2.0 ** 300)])
    fx = np.array([0.0, 0.0, -0.0, -0.0, 1.0, 1.0, 2.0 ** 300, 2.0 ** -300])
    x[-fx.size:], y[-fy.size:] = fx, fy
    # small angles: x > 0 and |y| <= 0.4 |x|, the relative bound's domain
    m = 1 << 17
    xs = spread(rng, m, -200, 200)
    ys = xs * (0.4 * rng.random_sample(m)) * np.ldexp(1.0, -rng.randint(0, 50, m)) * (rng.randint(0, 2, m) * 2.0 - 1.0)
    return {"x": x, "y": y}, {"x": xs, "y": ys}


def tiny_args(upper):
    """sin_tiny (upper = 4) / asin_tiny (upper = 1): |x| < 2^-13 in range; 2^-13, its lower neighbour and larger ones mixed in"""
    rng = np.random.RandomState(25 + int(upper))
    below = np.nextafter(TINY_LIMIT, 0)
    log = np.concatenate([spread(rng, 1 << 18, -1022, -13, signed=True), (rng.random_sample(1 << 10) * 2 - 1) * 2.0 ** -1022])
    edges = whole_waves([0.0, -0.0, below, -below, 5e-324, -5e-324, 2.0 ** -14, 2.0 ** -27, 2.0 ** -1022], 0.0)
    in_range = {"edges": edges, "log": log[: log.size // 64 * 64]}
    big = np.concatenate([[TINY_LIMIT, -TINY_LIMIT, np.nextafter(TINY_LIMIT, 1), float(upper), -float(upper), 0.5, 1e-3],
                          TINY_LIMIT + rng.random_sample(249) * (upper - TINY_LIMIT)])
    base = spread(rng, 64 * big.size, -60, -13, signed=True)
    mixed = base.copy()
    mixed[MIXED_LANE::64] = big
    # the lower neighbour of 2^-13 stays on the helper's own path: a wave of them, and one next to a library lane
    mixed[MIXED_LANE + 1::64] = below
    return in_range, {"mixed": mixed, "all_large": TINY_LIMIT + rng.random_sample(1 << 12) * (upper - TINY_LIMIT)}


def cos_cap_in_range(x):
    x = np.asarray(x, dtype=np.float64)
    return (x < COS_CAP_HI) & (x > COS_CAP_LO) & (np.abs(x + PIO2_1) >= COS_CAP_GAP)


def cos_cap_args():
    rng = np.random.RandomState(27)
    n = 1 << 18
    x = COS_CAP_LO + rng.random_sample(n) * (COS_CAP_HI - COS_CAP_LO)
    x[: n // 4] = -PIO2_1 + (rng.randint(0, 2, n // 4) * 2.0 - 1.0) * spread(rng, n // 4, -20, -1)   # towards -pi/2, log-uniform
    x = x[cos_cap_in_range(x)]
    lim = [np.nextafter(COS_CAP_LO, 0), np.nextafter(COS_CAP_HI, -1)]
    gap_lo, gap_hi = -PIO2_1 - COS_CAP_GAP, -PIO2_1 + COS_CAP_GAP     # exact sums: PIO2_1 has 33 bits
    lim += [gap_lo, np.nextafter(gap_lo, -2), gap_hi, np.nextafter(gap_hi, 0)]
    out = [COS_CAP_LO, COS_CAP_HI, np.nextafter(COS_CAP_LO, -3), np.nextafter(COS_CAP_HI, 0), np.nextafter(gap_lo, 0), np.nextafter(gap_hi, -2),
           -PIO2_1, -HALF_PI, 0.0, -0.0, 1.0, -3.0, 1e5, -1e22, np.inf, np.nan]
    in_range = {"limits": whole_waves(lim, -1.0), "bulk": x[: x.size // 64 * 64]}
    base = COS_CAP_LO + 0.01 + rng.random_sample(64 * len(out)) * 0.7
    mixed = base.copy()
    mixed[MIXED_LANE::64] = out
    return in_range, {"mixed": mixed, "all_outside": rng.random_sample(1 << 12) * 0.78}


def hom_arc_args():
    """s, w of OGG_MATH_HOM_ARC: |s| from 2^-40 to 1, w a power of two of either sign (the axis) in 2^-40 .. 2^40"""
    rng = np.random.RandomState(28)

    def w_of(n):
        return np.ldexp(1.0, rng.randint(-40, 41, n)) * (rng.randint(0, 2, n) * 2.0 - 1.0)

    n = 1 << 17
    s_small = spread(rng, n, -40, -10, signed=True)                       # all below 1e-3 (2^-10 = 9.8e-4)
    s_small[:8] = [2.0 ** -40, -2.0 ** -40, np.nextafter(ARC_SWITCH, 0), -np.nextafter(ARC_SWITCH, 0), 9.7e-4, 1e-6, 2e-6, -1e-4]
    s_mixed = spread(rng, n, -40, 0, signed=True)                         # both sides of the switch, lane by lane
    s_mixed[:8] = [1.0, -1.0, ARC_SWITCH, np.nextafter(ARC_SWITCH, 1), np.nextafter(ARC_SWITCH, 0), 0.5, 1e-3 + 1e-9, 2.0 ** -40]
    s_big = spread(rng, 1 << 12, -9, 0)                                   # all at or above the switch (2^-9 > 1e-3)
    s_zero = np.zeros(128)
    s_zero[1::2] = -0.0
    s_zero[64:] = s_small[:64]
    s_zero[64 + MIXED_LANE] = 0.0                                          # a zero among non-zeros: the early exit with the wave's ballot behind it
    return {"below": (s_small, w_of(n)), "mixed": (s_mixed, w_of(n)), "above": (s_big, w_of(s_big.size)), "zero": (s_zero, w_of(128))}


XCD_N = tuple(range(1, 301)) + tuple(v for k in range(1, 513) for v in (8 * k - 1, 8 * k + 1))


def xcd_contiguous_np(b, n):
    """numpy restatement of xcd_contiguous (ogg_math.h)"""
    b, n = np.asarray(b, dtype=np.int64), np.asarray(n, dtype=np.int64)
    x, r = b % 8, n % 8
    return x * (n // 8) + np.minimum(x, r) + b // 8
