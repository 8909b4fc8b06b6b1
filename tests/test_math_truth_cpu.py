"""The truth module behind tests/test_gpu_math_helpers.py, checked without a GPU: its two precision paths agree, its argument
generators stay inside the domains they name (the GPU tests drop nothing), and the numpy restatement of xcd_contiguous is the
renumbering the kernels rely on."""
import numpy as np
import pytest

import math_truth as mt

REL_AGREE = 2.0 ** -60


def _edge_lists():
    """name -> (x, y): the edge arguments of every helper, by the truth function that serves it"""
    rr = mt.rcp_rsqrt_args()["edges"]
    cap_in, cap_out = mt.atan_cap_args()
    sin_in, sin_out = mt.tiny_args(4)
    asin_in, asin_out = mt.tiny_args(1)
    cos_in, cos_out = mt.cos_cap_args()
    (gx, gy), (sx, sy) = [(d["x"], d["y"]) for d in mt.atan2_angle_args()]
    arc = mt.hom_arc_args()
    fin = lambda v: v[np.isfinite(v)]
    return {
        "rcp": (rr, None), "rsqrt": (rr, None),
        "atan": (np.concatenate([cap_in["edges"], fin(cap_out["mixed"][mt.MIXED_LANE::64]), np.abs(arc["below"][0][:8]), np.abs(arc["mixed"][0][:8])]), None),
        # the whole edge part of the general pairs (|y| = |x|, the neighbours of tan(pi/8), x = +-0, y = +-0: 4 x 4096 pairs behind the
        # comparable ones), the eight hand-made pairs at the end, and 4096 of the small angles
        "atan2": (np.concatenate([gx[1 << 17:(1 << 17) + 4 * 4096], gx[-8:], sx[:4096]]),
                  np.concatenate([gy[1 << 17:(1 << 17) + 4 * 4096], gy[-8:], sy[:4096]])),
        "sin": (np.concatenate([sin_in["edges"], sin_out["mixed"][:128]]), None),
        "asin": (np.concatenate([asin_in["edges"], asin_out["mixed"][:128]]), None),
        "cos": (np.concatenate([cos_in["limits"], fin(cos_out["mixed"][mt.MIXED_LANE::64])]), None),
    }


def test_longdouble_meets_the_precision_the_bulk_path_assumes_or_says_so():
    print("math_truth path on this machine: %s (longdouble eps %.3g)" % (mt.PATH, float(np.finfo(np.longdouble).eps)))
    assert mt.PATH in ("longdouble+mpmath-refined", "mpmath-subsample")
    assert mt.LONGDOUBLE_OK == (np.finfo(np.longdouble).eps <= 2.0 ** -63)


@pytest.mark.parametrize("name", mt.NAMES)
def test_longdouble_and_mpmath_agree_on_the_edge_lists(name):
    if not mt.LONGDOUBLE_OK:
        pytest.skip("no 80-bit long double here: the GPU tests take the mpmath path alone")
    x, y = _edge_lists()[name]
    assert x.size >= 16
    h1, l1 = mt.truth(name, x, y, "longdouble")
    h2, l2 = mt.truth(name, x, y, "mpmath")
    LD = np.longdouble
    d = np.abs((h1.astype(LD) - h2.astype(LD)) + (l1.astype(LD) - l2.astype(LD)))
    scale = np.abs(h2.astype(LD))
    ok = np.where(scale > 0, d <= REL_AGREE * scale, d == 0)
    assert ok.all(), (name, x[~ok][:5], None if y is None else y[~ok][:5])
    assert np.array_equal(np.signbit(h1), np.signbit(h2))


def test_hi_is_the_fp64_value_nearest_the_truth():
    x = np.array([0.1, 0.29, 1e-5, 2.0 ** -27])
    hi, lo = mt.truth("atan", x, None, "mpmath")
    assert np.all(np.abs(lo) <= 0.5 * mt.ulp_of(hi))
    assert np.array_equal(hi, np.arctan(x)) or np.max(np.abs(hi - np.arctan(x)) / mt.ulp_of(hi)) <= 1


def test_measure_sees_a_one_ulp_error_and_a_correct_rounding():
    rng = np.random.RandomState(3)
    x = mt.spread(rng, 4096, -20, 20)
    exact = 1.0 / x                                   # IEEE division: correctly rounded
    _, e = mt.measure("rcp", exact, x)
    assert e.max() <= 0.5
    _, e = mt.measure("rcp", np.nextafter(exact, np.inf), x)
    assert 0.5 <= e.min() and e.max() <= 1.5


def _whole_waves(d):
    for k, v in d.items():
        vs = v if isinstance(v, tuple) else (v,)
        for a in vs:
            assert a.dtype == np.float64 and a.size % 64 == 0 and a.size <= 1 << 20, k


def test_generators_stay_inside_the_domains_they_name():
    d = mt.div_pi180_args()
    assert d["arctan2_table"].size == 4096 and d["binades"].size == 1 << 20
    b = np.abs(d["binades"])
    assert b.min() >= 2.0 ** -1000 and b.max() < 2.0 ** 1000 and (d["binades"] < 0).any() and (d["binades"] > 0).any()
    assert np.abs(d["radians"]).max() <= 2 * np.pi
    z = d["zeros"]
    assert z[0] == 0 and not np.signbit(z[0]) and z[1] == 0 and np.signbit(z[1])
    t = d["arctan2_table"]
    assert np.isfinite(t).all() and (t == 0).any() and (np.signbit(t) & (t == 0)).any() and (np.abs(t) == np.pi / 4).any() and \
        (np.abs(t) == np.pi / 2).any() and (np.abs(t) == np.pi).any()

    r = mt.rcp_rsqrt_args()
    _whole_waves(r)
    for v in r.values():
        assert v.min() >= 2.0 ** -340 and v.max() <= 2.0 ** 340
    e = r["edges"]
    for p in (2.0 ** -340, 1.0, 4.0, 2.0 ** 340, 2.0 ** 101):
        assert p in e
    assert np.nextafter(4.0, 0) in e and np.nextafter(4.0, 5) in e and np.nextafter(2.0, 0) in e

    cap_in, cap_out = mt.atan_cap_args()
    _whole_waves(cap_in), _whole_waves(cap_out)
    for v in cap_in.values():
        assert v.min() >= 0.0 and v.max() <= mt.ATAN_CAP_LIMIT
    assert cap_in["log"].min() < 2.0 ** -1022 and 0.0 in cap_in["edges"] and 2.0 ** -27 in cap_in["edges"] and 0.3 in cap_in["edges"]
    assert np.nextafter(0.3, 0) in cap_in["edges"] and np.nextafter(0.3, 1) in cap_out["mixed"]
    m = cap_out["mixed"].reshape(-1, 64)
    out = ~(m <= mt.ATAN_CAP_LIMIT)
    assert out[:, mt.MIXED_LANE].all() and out.sum() == m.shape[0]            # exactly lane 17 of every wave
    assert np.isnan(cap_out["mixed"]).any() and (cap_out["all_above"] > mt.ATAN_CAP_LIMIT).all()

    g, s = mt.atan2_angle_args()
    _whole_waves(g), _whole_waves(s)
    for a in (g["x"], g["y"]):
        nz = np.abs(a[a != 0])
        assert np.isfinite(a).all() and nz.min() >= 2.0 ** -300 and nz.max() <= 2.0 ** 300
    assert (np.abs(g["x"]) == np.abs(g["y"])).sum() >= 4096
    zz = (g["x"] == 0) & (g["y"] == 0)
    assert sorted(set(zip(np.signbit(g["x"][zz]).tolist(), np.signbit(g["y"][zz]).tolist()))) == [(False, False), (False, True), (True, False), (True, True)]
    assert (s["x"] > 0).all() and (np.abs(s["y"]) <= 0.4 * s["x"]).all() and np.isfinite(s["y"]).all() and (np.abs(s["y"][s["y"] != 0]) >= 2.0 ** -300).all()

    for upper in (4, 1):
        t_in, t_out = mt.tiny_args(upper)
        _whole_waves(t_in), _whole_waves(t_out)
        for v in t_in.values():
            assert (np.abs(v) < mt.TINY_LIMIT).all()
        ed = t_in["edges"]
        assert np.signbit(ed[1]) and ed[1] == 0 and not np.signbit(ed[0]) and np.nextafter(mt.TINY_LIMIT, 0) in ed
        assert (t_in["log"] < 0).any() and np.abs(t_in["log"]).min() < 2.0 ** -1022
        big = np.abs(t_out["mixed"]) >= mt.TINY_LIMIT
        assert big.reshape(-1, 64)[:, mt.MIXED_LANE].all() and big.sum() == big.size // 64
        assert np.abs(t_out["mixed"]).max() == upper and mt.TINY_LIMIT in t_out["mixed"]
        assert (t_out["all_large"] >= mt.TINY_LIMIT).all() and (t_out["all_large"] <= upper).all()

    c_in, c_out = mt.cos_cap_args()
    _whole_waves(c_in), _whole_waves(c_out)
    for v in c_in.values():
        assert mt.cos_cap_in_range(v).all()
    assert c_in["bulk"].size >= 1 << 17 and np.abs(c_in["bulk"] + mt.PIO2_1).min() < 2.0 ** -19
    o = ~mt.cos_cap_in_range(c_out["mixed"]).reshape(-1, 64)
    assert o[:, mt.MIXED_LANE].all() and o.sum() == o.shape[0]
    assert not mt.cos_cap_in_range(c_out["all_outside"]).any()

    arc = mt.hom_arc_args()
    _whole_waves(arc)
    for k, (sv, wv) in arc.items():
        assert np.all(np.abs(sv) <= 1.0) and np.all((sv == 0) | (np.abs(sv) >= 2.0 ** -40)), k
        m_, e_ = np.frexp(np.abs(wv))
        assert np.all(m_ == 0.5) and np.all(np.abs(wv) >= 2.0 ** -40) and np.all(np.abs(wv) <= 2.0 ** 40), k
    assert (np.abs(arc["below"][0]) < mt.ARC_SWITCH).all() and (arc["above"][0] >= mt.ARC_SWITCH).all()
    mixed = np.abs(arc["mixed"][0]).reshape(-1, 64) >= mt.ARC_SWITCH
    assert (mixed.any(axis=1) & ~mixed.all(axis=1)).sum() > mixed.shape[0] // 2   # most waves hold lanes on both sides of the switch
    assert (arc["zero"][0][:64] == 0).all() and arc["zero"][0][64 + mt.MIXED_LANE] == 0


def test_xcd_contiguous_restated_is_a_bijection_that_gives_each_xcd_consecutive_indices():
    assert set(range(1, 301)) <= set(mt.XCD_N) and 4095 in mt.XCD_N and 4097 in mt.XCD_N and 7 in mt.XCD_N
    for n in mt.XCD_N:
        b = np.arange(n)
        v = mt.xcd_contiguous_np(b, n)
        assert np.array_equal(np.sort(v), b), n                                 # a renumbering of 0 .. n-1
        start = 0
        for x in range(8):
            mine = v[b % 8 == x]                                                # the workgroups of XCD x, in dispatch order
            assert np.array_equal(mine, start + np.arange(mine.size)), (n, x)   # consecutive, ascending, XCD after XCD
            start += mine.size
