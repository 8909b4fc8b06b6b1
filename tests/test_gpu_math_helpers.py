"""The scalar device helpers that DEPART from the library on purpose, one by one, against an extended-precision truth.

Every helper of csrc/ogg_math.h, ogg_bipolar_dev.h and ogg_dpole_dev.h that carries an accuracy or bit-identity claim in its comment
is evaluated through ogg_math_eval_dev (element k = thread k of 256-thread workgroups, so that the arrays below decide what each wave
of 64 lanes sees) and held to that claim: against tests/math_truth.py's hi + lo truth inside the helper's range, and bit for bit
against the device library's own function -- from the same build -- wherever the helper hands over to it.  A "mixed" array holds an
out-of-range argument in lane 17 of every wave: the helpers that choose by a ballot must then give the library's bits in EVERY lane.

Every measured worst case goes to math_helpers.json in the run's output directory, next to test_gpu_truth.py's table (copied to
profiles/math_helpers.json, tabulated in DESIGN.md section 2).
"""
import json
import os

import numpy as np
import pytest

import math_truth as mt
from oracle import ogg_oracle as orc

pytestmark = pytest.mark.gpu

REPORT = {"truth_path": mt.PATH}
LANE = mt.MIXED_LANE


def _report_dir():
    """The directory test_gpu_truth.py writes its table to (the name is read from its _save, so that the two reports cannot part)"""
    import inspect
    import re

    import test_gpu_truth
    name = re.search(r'"(\w+_out)"', inspect.getsource(test_gpu_truth._save)).group(1)
    return os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), name)


def _save():
    d = _report_dir()
    try:
        os.makedirs(d, exist_ok=True)
        with open(os.path.join(d, "math_helpers.json"), "w") as f:
            json.dump(REPORT, f, indent=1, sort_keys=True)
    except OSError:
        pass


def record(key, **figures):
    REPORT.setdefault(key, {}).update({k: (float(v) if isinstance(v, (float, np.floating)) else int(v)) for k, v in figures.items()})
    print(key, REPORT[key])
    _save()


def ev(hip, name, x, y=None):
    """out[k] = helper(x[k][, y[k]]) on the device, as a numpy array"""
    import torch
    xt = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64)).cuda()
    yt = None if y is None else torch.from_numpy(np.ascontiguousarray(y, dtype=np.float64)).cuda()
    out = torch.full_like(xt, float("nan"))
    hip.call("ogg_math_eval_dev", hip.MATH[name], xt.numel(), xt.data_ptr(), None if yt is None else yt.data_ptr(), out.data_ptr(),
             torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    return int((bits(a) != bits(b)).sum())


def worst(name, v, x, y=None, relative_to="ulp"):
    """(worst error, its argument index, number of arguments measured)"""
    idx, err = mt.measure(name, v, x, y, keep=np.arange(min(64, np.size(x))), relative_to=relative_to)
    k = int(np.argmax(err))
    return float(err[k]), int(idx[k]), int(idx.size)


# ---------------------------------------------------------------------------------------------------------------
# ogg_math.h
# ---------------------------------------------------------------------------------------------------------------
def test_div_pi180_is_the_ieee_division_bit_for_bit_sign_of_zero_included(hip):
    """div_pi180(a) against numpy's a / (numpy.pi / 180), compared as BYTES: both signed zeros, 2^20 operands of either sign over
    2^-1000 .. 2^1000, the radians range +-2 pi densely, every value numpy.arctan2 takes on a 64 x 64 table of signed zeros, equal
    magnitudes and axis points.  (With the residual as it was before it was negated, -0.0 came back as +0.0 and this test failed at "zeros".)"""
    for key, a in mt.div_pi180_args().items():
        got = ev(hip, "div_pi180", a)
        want = a / mt.PI_180
        n = same_bits(got, want)
        record("div_pi180/" + key, n=a.size, n_diff=n)
        assert n == 0, (key, a[bits(got) != bits(want)][:8])


@pytest.mark.parametrize("helper,name,bound", [("rcp_c3", "rcp", 0.501), ("rsqrt_c3", "rsqrt", 1.0)])
def test_rcp_c3_and_rsqrt_c3_meet_their_ulp_bounds(hip, helper, name, bound):
    """Positive normal x over the 680 binades 2^-340 .. 2^340, the powers of two (and so of four) with their neighbours.  rcp_c3 <= 0.501
    ulp: the final fma's 0.5 ulp plus e^3 of truncation, below 1e-3 ulp for any seed error up to 2^-21; rsqrt_c3 <= 1.0 ulp, the comment's
    own figure."""
    for key, x in mt.rcp_rsqrt_args().items():
        v = ev(hip, helper, x)
        e, k, n = worst(name, v, x)
        record("%s/%s" % (helper, key), n=n, max_ulp=e, at=x[k])
        assert e <= bound, (key, e, x[k])


def test_wave_prev_and_wave_next_move_whole_doubles_and_keep_the_end_lanes(hip):
    """Distinct values that differ only in the LOW word, then only in the HIGH word (a shift that moved one word alone would show):
    lane l gets lane l -+ 1's value, lanes 0 / 63 keep their own.  n = 64 * 9 + 37: three workgroups and a last wave of 37 elements --
    in uniform control flow (the threads behind n recompute element n - 1) and with those threads returned before the shift (_tail):
    the last element's right neighbour is then an inactive lane, and wave_next leaves the lane its own value."""
    n = 64 * 9 + 37
    k = np.arange(n, dtype=np.uint64)
    for word, x in (("low", (np.uint64(0x3FF0000000000000) + k + np.uint64(1)).view(np.float64)),
                    ("high", ((np.uint64(0x3FF00000) + k + np.uint64(1)) << np.uint64(32)).view(np.float64))):
        assert np.unique(x).size == n
        prev, nxt = x.copy(), x.copy()
        prev[1:] = x[:-1]
        nxt[:-1] = x[1:]
        prev[0::64] = x[0::64]
        nxt[63::64] = x[63::64]
        for code, want in (("wave_prev", prev), ("wave_next", nxt), ("wave_prev_tail", prev), ("wave_next_tail", nxt)):
            got = ev(hip, code, x)
            d = same_bits(got, want)
            record("%s/%s_word" % (code, word), n=n, n_diff=d)
            assert d == 0, (code, word, np.nonzero(bits(got) != bits(want))[0][:8])
    # the int overload of wave_next (one word, the same DPP control): distinct integers held in doubles
    xi = (np.arange(n) * 7919 % 100003 - 50000).astype(np.float64)
    assert np.unique(xi).size == n
    want = xi.copy()
    want[:-1] = xi[1:]
    want[63::64] = xi[63::64]
    got = ev(hip, "wave_next_int", xi)
    d = int((got != want).sum())
    record("wave_next_int", n=n, n_diff=d)
    assert d == 0


def test_xcd_contiguous_equals_its_numpy_restatement(hip):
    """Every b of every n = 1 .. 300 and 8k +- 1 up to 1025; the ends and 256 random b of each 8k +- 1 up to 4097 (the restatement itself is
    shown to be the wanted renumbering in test_math_truth_cpu.py)."""
    rng = np.random.RandomState(5)
    bs, ns = [], []
    for n in mt.XCD_N:
        b = np.arange(n) if n <= 1025 else np.unique(np.concatenate([np.arange(16), n - 1 - np.arange(16), rng.randint(0, n, 256)]))
        bs.append(b), ns.append(np.full(b.size, n))
    b, n = np.concatenate(bs), np.concatenate(ns)
    assert b.size <= 1 << 20
    got = ev(hip, "xcd_contiguous", b.astype(np.float64), n.astype(np.float64))
    want = mt.xcd_contiguous_np(b, n)
    d = int((got != want.astype(np.float64)).sum())
    record("xcd_contiguous", n=b.size, n_diff=d)
    assert d == 0


# ---------------------------------------------------------------------------------------------------------------
# ogg_bipolar_dev.h
# ---------------------------------------------------------------------------------------------------------------
def test_atan_cap_meets_its_bound_in_range_and_is_the_library_outside(hip):
    """u in [0, 0.3] uniform, log-uniform down to the subnormals, 0, 2^-27, 0.3 and its lower neighbour: <= 0.57 ulp, and the same
    bits as the bare 14-term series (atan_series<14>).  A wave that holds the upper neighbour of 0.3, a larger argument, an infinity or a
    NaN in lane 17: the device library's atan, bit for bit, in all 64 lanes."""
    in_range, outside = mt.atan_cap_args()
    for key, u in in_range.items():
        v = ev(hip, "atan_cap", u)
        e, k, n = worst("atan", v, u)
        d = same_bits(v, ev(hip, "atan_series14", u))
        record("atan_cap/" + key, n=n, max_ulp=e, at=u[k], n_diff_series14=d)
        assert e <= 0.57, (key, e, u[k])
        assert d == 0
        assert not np.signbit(v).any()
    for key, u in outside.items():
        d = same_bits(ev(hip, "atan_cap", u), ev(hip, "lib_atan", u))
        record("atan_cap/" + key, n=u.size, n_diff_library=d)
        assert d == 0, key
    # the restatement the other helpers fall back to is the library too, on these arrays
    u = outside["mixed"]
    assert same_bits(ev(hip, "atan_lib", u), ev(hip, "lib_atan", u)) == 0


def test_atan_series17_stays_inside_the_absolute_bound_of_the_angle_it_serves(hip):
    """|r| <= tan(pi/8), the reduced argument of atan2_angle: the 17-term series may not use up more than atan2_angle's own 6e-16 rad (the
    first omitted term alone is r^37 / 37 = 6e-17 rad at the end of the range).  The figure in ulps is recorded, not bounded: the series is
    not a <1 ulp function at the end of its range and is not used as one."""
    rng = np.random.RandomState(31)
    r = np.concatenate([(rng.random_sample(1 << 17) * 2 - 1) * mt.TAN_PI_8, [mt.TAN_PI_8, -mt.TAN_PI_8, 0.0, -0.0, 1e-300, 2.0 ** -27], np.zeros(58)])
    v = ev(hip, "atan_series17", r)
    e, k, n = worst("atan", v, r, relative_to="abs")
    eu, ku, _ = worst("atan", v, r)
    record("atan_series17", n=n, max_abs=e, at=r[k], max_ulp=eu, ulp_at=r[ku])
    assert e <= 6e-16
    nz = r != 0                                                # (the bare series returns +0.0 for -0.0; atan2_angle takes its sign from y)
    assert np.array_equal(np.signbit(v[nz]), np.signbit(r[nz])) and not v[~nz].any()


def test_atan2_angle_absolute_and_small_angle_bounds_and_the_sign_of_y(hip):
    """Finite pairs of either sign, magnitudes 2^-300 .. 2^300 and comparable ones in +-2, |y| = |x|, the neighbours of mn = tan(pi/8) mx,
    x = 0, y = 0, the four signed-zero pairs: <= 6e-16 rad absolute (the comment), the sign bit of y.  At the origin the truth is the
    helper's documented 0.  Where x > 0 and |y| <= 0.4 |x|: <= 4 ulp of the true angle -- one reciprocal of <= 1 ulp, one product, one
    fma, a factor 1.5 of room -- because an absolute bound alone would let small angles come out as zero."""
    general, small = mt.atan2_angle_args()
    x, y = general["x"], general["y"]
    v = ev(hip, "atan2_angle", x, y)
    e, k, n = worst("atan2", v, x, y, relative_to="abs")
    record("atan2_angle/general", n=n, max_abs=e, at_x=x[k], at_y=y[k])
    assert e <= 6e-16, (e, x[k], y[k])
    assert np.array_equal(np.signbit(v), np.signbit(y))
    x, y = small["x"], small["y"]
    v = ev(hip, "atan2_angle", x, y)
    e, k, n = worst("atan2", v, x, y)
    ea, _, _ = worst("atan2", v, x, y, relative_to="abs")
    record("atan2_angle/small", n=n, max_ulp=e, at_x=x[k], at_y=y[k], max_abs=ea)
    assert e <= 4.0, (e, x[k], y[k])
    assert ea <= 6e-16
    assert np.array_equal(np.signbit(v), np.signbit(y))


# ---------------------------------------------------------------------------------------------------------------
# ogg_dpole_dev.h
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("helper,name,lib,upper", [("sin_tiny", "sin", "lib_sin", 4), ("asin_tiny", "asin", "lib_asin", 1)])
def test_sin_tiny_and_asin_tiny(hip, helper, name, lib, upper):
    """|x| < 2^-13, log-uniform to the subnormals, both signs: <= 0.5001 ulp, and a zero keeps its sign (bytes).  2^-13 itself, its lower
    neighbour and larger arguments (sin to 4, asin to 1): the device library's bits -- these two helpers choose lane by lane, so in a mixed
    wave the small lanes keep the series and its bound."""
    in_range, outside = mt.tiny_args(upper)
    for key, x in in_range.items():
        v = ev(hip, helper, x)
        e, k, n = worst(name, v, x)
        record("%s/%s" % (helper, key), n=n, max_ulp=e, at=x[k])
        assert e <= 0.5001, (key, e, x[k])
        z = x == 0
        assert same_bits(v[z], x[z]) == 0                       # +-0 -> +-0
        assert np.array_equal(np.signbit(v), np.signbit(x))
    below = np.nextafter(mt.TINY_LIMIT, 0)
    edge = mt.whole_waves([below, -below, mt.TINY_LIMIT, -mt.TINY_LIMIT], below)
    d = same_bits(ev(hip, helper, edge), ev(hip, lib, edge))
    record(helper + "/edge", n_diff_library=d)
    assert d == 0
    x = outside["all_large"]
    d = same_bits(ev(hip, helper, x), ev(hip, lib, x))
    record(helper + "/all_large", n=x.size, n_diff_library=d)
    assert d == 0
    x = outside["mixed"]
    v, vl = ev(hip, helper, x), ev(hip, lib, x)
    big = np.abs(x) >= mt.TINY_LIMIT
    d = same_bits(v[big], vl[big])
    e, k, n = worst(name, v[~big], x[~big])
    record(helper + "/mixed", n=x.size, n_diff_library=d, max_ulp_small_lanes=e)
    assert d == 0 and e <= 0.5001


def test_cos_cap_meets_its_bound_in_range_and_is_the_library_outside(hip):
    """x in (-3 pi/4, -pi/4) outside 2^-20 of -pi/2, log-uniform towards -pi/2, the neighbours of all four limits: <= 0.73 ulp.  A wave
    with a lane outside (the limits themselves, their outer neighbours, -pi/2, zeros, huge arguments, an infinity, a NaN): the device
    library's cos in all 64 lanes."""
    in_range, outside = mt.cos_cap_args()
    for key, x in in_range.items():
        v = ev(hip, "cos_cap", x)
        e, k, n = worst("cos", v, x)
        record("cos_cap/" + key, n=n, max_ulp=e, at=x[k])
        assert e <= 0.73, (key, e, x[k])
    for key, x in outside.items():
        d = same_bits(ev(hip, "cos_cap", x), ev(hip, "lib_cos", x))
        record("cos_cap/" + key, n=x.size, n_diff_library=d)
        assert d == 0, key


def test_homogeneous_arc_on_the_family_with_exact_cross_products(hip):
    """a = (0, 0, w), b = (s w, 0, w) or (0, s w, w), w a power of two: tan(theta) = |s| exactly, the truth is atan|s|.  Relative error <=
    2^-49 (2^-50 for the root, plus the roundings of cc * y and of the series) for |s| from 2^-40 to 1 -- arrays wholly below the switch
    at t = 1e-3, wholly above, and mixed lane by lane --; a lane with t >= 1e-3 is atan_lib of the DEVICE's own t within that bound; s = 0
    gives 0, alone and among non-zero lanes."""
    bound = 2.0 ** -49
    for key, (s, w) in mt.hom_arc_args().items():
        th = ev(hip, "hom_arc", s, w)
        t = ev(hip, "hom_tan", s, w)
        assert not np.signbit(th).any()
        zero = s == 0
        assert same_bits(th[zero], np.zeros(int(zero.sum()))) == 0
        nz = ~zero
        e, k, n = worst("atan", th[nz], np.abs(s[nz]), relative_to="rel")
        et = float(np.max(np.abs(t[nz] - np.abs(s[nz])) / np.abs(s[nz])))
        lib = t >= mt.ARC_SWITCH
        el, n_bits = 0.0, 0
        if lib.any():
            a = ev(hip, "atan_lib", mt.whole_waves(t[lib], 1.0))[: int(lib.sum())]
            el = float(np.max(np.abs(th[lib] - a) / a))
            n_bits = same_bits(th[lib], a)
        record("homogeneous_arc/" + key, n=n, max_rel=e, at=s[nz][k], max_rel_tan=et, n_library_lanes=int(lib.sum()), max_rel_vs_atan_lib=el,
               n_diff_atan_lib=n_bits)
        assert e <= bound, (key, e, s[nz][k])
        assert el <= bound
        if key == "below":
            assert not lib.any()
        if key == "above":
            assert lib.all()


# ---------------------------------------------------------------------------------------------------------------
# the sign of a zero angle, end to end
# ---------------------------------------------------------------------------------------------------------------
def test_angle_x_of_signed_zero_latitudes_equals_the_oracle_byte_for_byte(hip):
    """ogg.angle_x on a caller's mesh whose latitudes are zeros of either sign, so that differences of -0.0 occur in the interior and at
    both ends of a row (and, in the last row, next to longitudes that run backwards: +-180).  The oracle's arctan2(-0.0, positive) / PI_180
    is -0.0; assert_array_equal cannot tell it from +0.0, the bytes can.  (With div_pi180's residual as it was: 98 of the 420 values differ, every -0.0 of the oracle.)"""
    import ocean_model_grid_generator_amd.ocean_grid_generator as ogg
    rng = np.random.RandomState(7)
    nj1, ni1 = 6, 70
    x = np.cumsum(0.5 + rng.random_sample((nj1, ni1)), axis=1) - 300.0
    x[-1] = x[-1, ::-1]
    y = np.where(rng.randint(0, 2, (nj1, ni1)) == 1, -0.0, 0.0)
    y[:, 0], y[:, 1] = 0.0, -0.0                 # y[1] - y[0] = -0.0 at the left end
    y[:, -2], y[:, -1] = 0.0, -0.0               # y[-1] - y[-2] = -0.0 at the right end
    y[0, 10], y[0, 12] = 0.0, -0.0               # ... and at an interior column
    want = orc.angle_x(x, y)
    neg = np.signbit(want) & (want == 0)
    assert neg[:-1, 0].all() and neg[:-1, -1].all() and neg[:-1, 1:-1].any() and (~neg[:-1, 1:-1]).any()
    assert set(np.unique(np.abs(want[-1]))) == {180.0}
    got = ogg.angle_x(x, y)
    d = same_bits(got, want)
    record("angle_x_signed_zero", n=want.size, n_negative_zero=int(neg.sum()), n_diff=d)
    assert got.tobytes() == want.tobytes()


@pytest.mark.parametrize("sym", [pytest.param(1, id="mirror"), pytest.param(2, id="every_column")])
def test_bipolar_mesh_angle_of_the_row_of_equal_latitudes_is_plus_zero_at_mirrored_columns_too(hip, sym):
    """Row j = 0 of a bipolar cap lies on one latitude: the reference's angle_x is +0.0 at every column.  The mesh kernel writes the
    NEGATED angle to two of a column's three mirror images; the negative of +0.0 must not reach the file (0 - a, not -a: with -a, 170 of
    the 361 values of the row were -0.0).  Only the mirrored case exercises those stores; every_column is the control -- the same row from
    columns evaluated one by one -- and held +0.0 before the change too.  The fused pass inlines the same bipolar_mesh_body."""
    import torch
    Ni, Nj, lat0, lon_bp, nrows = 360, 8, 66.0, -300.0, 2
    lams, phis = orc.generate_bipolar_cap_mesh(Ni, Nj, lat0, lon_bp)[:2]
    want = orc.angle_x(lams, phis)[:nrows]
    assert want[0].tobytes() == np.zeros(Ni + 1).tobytes()
    bufs = [torch.full((nrows, Ni + 1), float("nan"), dtype=torch.float64, device="cuda:0") for _ in range(3)]
    hip.call("ogg_bipolar_cap_mesh_angle_sym_dev", Ni, Nj, lat0, lon_bp, 0, nrows, sym, bufs[0].data_ptr(), bufs[1].data_ptr(), None, None,
             bufs[2].data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = bufs[2].cpu().numpy()
    record("bipolar_mesh_angle_row0/sym%d" % sym, n_negative_zero=int((np.signbit(got[0]) & (got[0] == 0)).sum()), n_nonzero=int((got[0] != 0).sum()))
    assert got[0].tobytes() == want[0].tobytes()
    assert np.max(np.abs(got[1] - want[1])) < 1e-9
