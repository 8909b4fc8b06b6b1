"""CPU tests of the basin codes (no GPU): the box predicate of the definition in tests/basin_definition.py and of the library's host
check at its edges, the rule file, the refusals of ogg_basin_check, the pass planner, main()'s flag validation, and the definition on
a hand-made case where the order of two overlapping rules decides the result."""
import numpy as np
import pytest

import basin_definition as D
import small_meshes as SM
from ocean_model_grid_generator_amd import basin_codes as BC


def rule(code=1, seed=(0.0, 0.0), box=(-10.0, 10.0, -10.0, 10.0), name=None):
    r = (code, seed[0], seed[1]) + tuple(box)
    return r + (name,) if name is not None else r


def lib_in_box(lon, lat, box):
    """the library's own host predicate, through the seed-in-its-box check of ogg_basin_check"""
    try:
        BC.params(4, 4, BC.rules_of([rule(1, (lon, lat), box)]))
        return True
    except ValueError as e:
        assert "lies outside its box" in str(e)
        return False


# ---- the predicate -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lon, want", [(5.0, True), (365.0, True), (-355.0, True), (350.0, True), (370.0, True), (10.0, True),
                                       (-350.0, True), (730.0, True), (349.0, False), (11.0, False), (180.0, False),
                                       (np.nextafter(350.0, 0.0), False), (10.0 + 1e-9, False)])
def test_a_box_across_the_seam_holds_centres_stated_on_any_turn(lon, want):
    box = (350.0, 370.0, -5.0, 5.0)
    assert bool(D.in_box(lon, 0.0, *box)) is want
    assert lib_in_box(lon, 0.0, box) is want


def test_t_that_rounds_to_360_is_in_the_box_only_when_w_is_360():
    lon = -1.0e-20   # t = -1e-20, floor(t / 360) = -1, t + 360 rounds to exactly 360.0
    t = lon - 0.0
    assert t - 360.0 * np.floor(t / 360.0) == 360.0
    assert not D.in_box(lon, 0.0, 0.0, 20.0, -5.0, 5.0) and not lib_in_box(lon, 0.0, (0.0, 20.0, -5.0, 5.0))
    assert not D.in_box(lon, 0.0, 0.0, np.nextafter(360.0, 0.0), -5.0, 5.0)
    assert D.in_box(lon, 0.0, 0.0, 360.0, -5.0, 5.0) and lib_in_box(lon, 0.0, (0.0, 360.0, -5.0, 5.0))


def test_a_full_turn_holds_every_longitude():
    lon = np.array([-1.0e9, -720.0, -180.0, -1e-300, 0.0, 17.25, 359.999, 360.0, 1.0e9])
    assert np.all(D.in_box(lon, 0.0, -180.0, 180.0, -5.0, 5.0))
    assert all(lib_in_box(float(v), 0.0, (-180.0, 180.0, -5.0, 5.0)) for v in lon)
    assert not D.in_box(0.0, 5.1, -180.0, 180.0, -5.0, 5.0)


def test_a_centre_on_each_edge_is_in_the_box():
    box = (20.0, 47.5, -33.25, 12.0)
    for lon, lat in ((20.0, 0.0), (47.5, 0.0), (30.0, -33.25), (30.0, 12.0), (20.0, -33.25), (47.5, 12.0)):
        assert D.in_box(lon, lat, *box) and lib_in_box(lon, lat, box)
    for lon, lat in ((np.nextafter(20.0, 0.0), 0.0), (np.nextafter(47.5, 99.0), 0.0), (30.0, np.nextafter(-33.25, -99.0)),
                     (30.0, np.nextafter(12.0, 99.0))):
        assert not D.in_box(lon, lat, *box) and not lib_in_box(lon, lat, box)
    assert not D.in_box(np.nan, 0.0, *box) and not D.in_box(30.0, np.nan, *box)


# ---- the rule file -------------------------------------------------------------------------------------------------
def test_rule_file(tmp_path):
    f = tmp_path / "rules.txt"
    f.write_text("# code seed box [name]\n"
                 "1 -30 -60 -180 180 -90 -35 southern   # the ring\n"
                 "\n"
                 "2 -30.5 10 -70 20 -35 65 atlantic\n"
                 "2 -60 25 -100 -50 5 35\n"
                 "3 1e1 2.5e1 0 40 20 45\n")
    r = BC.read_rules(str(f))
    assert len(r) == 4 and r.names == ["southern", "atlantic", "atlantic", None]
    assert r.table["code"].tolist() == [1, 2, 2, 3] and r.table["seed_lon"].tolist() == [-30.0, -30.5, -60.0, 10.0]
    assert r.table["lon_w"].tolist() == [-180.0, -70.0, -100.0, 0.0] and r.table["lat_n"].tolist() == [-35.0, 65.0, 35.0, 45.0]
    assert r.table.dtype.itemsize == 56
    for text, what in (("1 0 0 -10 10 -10\n", "6 values"), ("1 0 0 -10 10 -10 10 a b\n", "9 values"), ("x 0 0 -10 10 -10 10\n", "integer code"),
                       ("1.5 0 0 -10 10 -10 10\n", "integer code"), ("1 0 zero -10 10 -10 10\n", "six numbers"), ("# nothing\n\n", "no rules"),
                       ("1 0 0 -10 10 -10 10 a\n1 0 5 -10 10 -10 10 b\n", "is named a and b")):
        f.write_text(text)
        with pytest.raises(ValueError, match=what):
            BC.read_rules(str(f))
    with pytest.raises(ValueError, match="has 6 values"):
        BC.rules_of([(1, 0, 0, -10, 10, -10)])
    with pytest.raises(ValueError, match="not an integer"):
        BC.rules_of([(float("nan"), 0, 0, -10, 10, -10, 10)])


# ---- the library's checks ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rules, what", [
    ([rule(0)], "code 0"), ([rule(256)], "code 256"), ([rule(-1)], "code -1"),
    ([rule(box=(10.0, 10.0, -10.0, 10.0), seed=(10.0, 0.0))], "lon_e - lon_w"), ([rule(box=(10.0, -10.0, -10.0, 10.0))], "lon_e - lon_w"),
    ([rule(box=(-180.0, 180.5, -10.0, 10.0))], "lon_e - lon_w"),
    ([rule(box=(-10.0, 10.0, 10.0, -10.0))], "lat_s <= lat_n"), ([rule(box=(-10.0, 10.0, -91.0, 10.0))], "lat_s <= lat_n"),
    ([rule(box=(-10.0, 10.0, -10.0, 90.5))], "lat_s <= lat_n"),
    ([rule(seed=(11.0, 0.0))], "rule 0: the seed"), ([rule(), rule(seed=(0.0, 10.5))], "rule 1: the seed"),
    ([rule(seed=(float("nan"), 0.0))], "not finite"), ([rule(seed=(0.0, float("inf")))], "not finite"),
    ([rule(box=(float("nan"), 10.0, -10.0, 10.0))], "not finite"), ([rule(box=(-10.0, float("nan"), -10.0, 10.0))], "not finite"),
    ([rule(box=(-10.0, 10.0, float("nan"), 10.0))], "not finite"), ([rule(), rule(box=(-10.0, 10.0, -10.0, float("-inf")))], "rule 1 holds"),
    ([], "0 rules"), ([rule()] * 4097, "4097 rules"),
])
def test_check_refuses(rules, what):
    with pytest.raises(ValueError, match=what):
        BC.params(4, 4, BC.rules_of(rules))


def test_check_accepts_the_limits_and_refuses_bad_sizes():
    BC.params(4, 4, BC.rules_of([rule(255, box=(-180.0, 180.0, -90.0, 90.0))] * 4096))
    BC.params(1, 1, BC.rules_of([rule(1, (5.0, 5.0), (5.0, 6.0, 5.0, 5.0))]))   # lat_s == lat_n, the seed on a corner
    with pytest.raises(ValueError, match="cells"):
        BC.params(0, 4, BC.rules_of([rule()]))
    with pytest.raises(ValueError, match="2\\^31"):
        BC.params(1 << 16, 1 << 15, BC.rules_of([rule()]))
    with pytest.raises(ValueError, match="seed_max_distance"):
        BC.params(4, 4, BC.rules_of([rule()]), seed_max_distance=-1.0)
    assert BC.seed_max_d2(None) == float("inf") and BC.seed_max_d2(0.0) == 0.0
    assert BC.seed_max_d2(1000.0e3, 6371.0e3) == (2.0 * np.sin(1000.0e3 / (2.0 * 6371.0e3))) ** 2


def test_struct_sizes():
    from ocean_model_grid_generator_amd import _lib as L
    import ctypes
    lib = L.load()
    assert lib.ogg_abi_sizeof(L.ABI["BASIN_PARAMS"]) == ctypes.sizeof(L.BasinParams) == 32
    assert lib.ogg_abi_sizeof(L.ABI["BASIN_RULE"]) == L.BASIN_RULE.itemsize == 56
    assert lib.ogg_abi_sizeof(L.ABI["BASIN_RULE_RECORD"]) == L.BASIN_RECORD.itemsize == D.RECORD.itemsize == 32
    assert lib.ogg_abi_sizeof(L.ABI["BASIN_COUNTS"]) == ctypes.sizeof(L.BasinCounts) == 32
    assert L.BASIN_RECORD == D.RECORD


# ---- the planner ---------------------------------------------------------------------------------------------------
def random_rules(rng, n):
    out = []
    for _ in range(n):
        w, s = 0.25 * rng.integers(-800, 800), 0.25 * rng.integers(-360, 320)   # (quarters: lon_e - lon_w is exact)
        W, H = rng.choice([5.0, 20.0, 90.0, 360.0]), rng.choice([0.0, 10.0, 60.0])
        e, nn = w + W, min(90.0, s + H)
        out.append((int(rng.integers(1, 256)), w + 0.5 * W, 0.5 * (s + nn), w, e, s, nn))
    return out


def check_plan(rules, start):
    assert start[0] == 0 and start[-1] == len(rules) and all(0 < b - a <= 255 for a, b in zip(start, start[1:]))   # a partition, in order
    for a, b in zip(start, start[1:]):
        for q in range(a, b):
            for r in range(q + 1, b):
                assert D.disjoint(rules[q], rules[r]) and D.disjoint(rules[r], rules[q]), (q, r)
                assert not D.boxes_share_a_point(rules[q], rules[r]) and not D.boxes_share_a_point(rules[r], rules[q])


def test_planner_partitions_in_order_into_pairwise_disjoint_passes(monkeypatch):
    rng = np.random.default_rng(3)
    batched = 0
    for _ in range(30):
        rules = random_rules(rng, 40)
        start = BC.plan(rules)
        check_plan(rules, start)
        batched += len(rules) - (len(start) - 1)
        # greedy: the rule that starts a pass is not disjoint from some rule of the pass before it (or that pass is full)
        for a, b in zip(start, start[1:-1]):
            assert b - a == 255 or any(not D.disjoint(rules[q], rules[b]) for q in range(a, b))
    assert batched > 100   # the planner does batch
    monkeypatch.setenv("OGG_BASIN_BATCH", "0")
    assert BC.plan(rules) == list(range(41))
    monkeypatch.setenv("OGG_BASIN_BATCH", "2")
    with pytest.raises(Exception, match="OGG_BASIN_BATCH"):
        BC.plan(rules)


def test_boxes_that_touch_or_nearly_touch_start_a_new_pass():
    a = rule(1, (5.0, 5.0), (0.0, 10.0, 0.0, 10.0))
    for b, passes in ((rule(2, (15.0, 5.0), (10.0, 20.0, 0.0, 10.0)), 2),            # share the meridian 10
                      (rule(2, (5.0, 15.0), (0.0, 10.0, 10.0, 20.0)), 2),            # share the parallel 10
                      (rule(2, (15.0, 5.0), (10.0 + 5e-10, 20.0, 0.0, 10.0)), 2),    # closer than 1e-9 degrees
                      (rule(2, (5.0, 15.0), (0.0, 10.0, 10.0 + 5e-10, 20.0)), 2),
                      (rule(2, (-345.0, 5.0), (-349.0, -340.0, 0.0, 10.0)), 1),      # 11 .. 20 stated a turn away: clear of 0 .. 10
                      (rule(2, (-345.0, 5.0), (-350.0, -340.0, 0.0, 10.0)), 2),      # 10 .. 20 stated a turn away: touches
                      (rule(2, (365.0, 5.0), (360.0, 380.0, 0.0, 10.0)), 2),         # the same box a turn away
                      (rule(2, (355.0, 5.0), (350.0, 360.0, 0.0, 10.0)), 2),         # touches across the seam
                      (rule(2, (355.0, 5.0), (350.0, 359.0, 0.0, 10.0)), 1),
                      (rule(2, (15.0, 5.0), (10.001, 20.0, 0.0, 10.0)), 1),
                      (rule(2, (5.0, 15.0), (0.0, 10.0, 10.001, 20.0)), 1),
                      (rule(2, (100.0, 5.0), (-180.0, 180.0, 0.0, 10.0)), 2),        # a full turn meets every arc
                      (rule(2, (100.0, 50.0), (-180.0, 180.0, 10.001, 90.0)), 1)):
        assert len(BC.plan([a, b])) - 1 == passes, b
        assert len(BC.plan([b, a])) - 1 == passes, b
        assert D.disjoint(a, b) == (passes == 1)


def test_a_pass_holds_at_most_255_rules():
    rules = [rule(1 + k % 255, (k + 0.5, 0.0), (k + 0.25, k + 0.75, -1.0, 1.0)) for k in range(300)]
    assert BC.plan(rules) == [0, 255, 300]
    assert BC.plan(rules[:255]) == [0, 255] and BC.plan(rules[:256]) == [0, 255, 256]


# ---- main()'s flags ------------------------------------------------------------------------------------------------
def test_main_refuses_incomplete_basin_flags_before_any_device_work():
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    for path in ("pass", "functions"):
        with pytest.raises(ValueError, match="--basin_codes_file needs --basin_rules"):
            ogg.main(1.0, gridfilename=None, basin_codes_file="b.nc", topog_source="t.nc", path=path)
        with pytest.raises(ValueError, match="--basin_codes_file needs --topog_source"):
            ogg.main(1.0, gridfilename=None, basin_codes_file="b.nc", basin_rules="r.txt", path=path)
        with pytest.raises(ValueError, match="need --basin_codes_file"):
            ogg.main(1.0, gridfilename=None, basin_rules="r.txt", topog_source="t.nc", path=path)
        with pytest.raises(ValueError, match="need --basin_codes_file"):
            ogg.main(1.0, gridfilename=None, basin_seed_max_km=100.0, path=path)
        with pytest.raises(ValueError, match="--basin_seed_max_km must be >= 0"):
            ogg.main(1.0, gridfilename=None, basin_codes_file="b.nc", basin_rules="r.txt", topog_source="t.nc", basin_seed_max_km=-1.0,
                     path=path)
    ogg._validate_all((), 0.0, -99.0, True, ogg.AnalysisFlags(basin_codes_file="b.nc", basin_rules="r.txt", topog_source="t.nc"))
    a = ogg.AnalysisFlags()
    assert a.basin_codes_file is None and a.basin_rules is None and a.basin_seed_max_km is None
    args = ogg.build_parser().parse_args(["-r", "1", "--basin_codes_file", "b.nc", "--basin_rules", "r.txt", "--basin_seed_max_km", "50"])
    assert (args.basin_codes_file, args.basin_rules, args.basin_seed_max_km) == ("b.nc", "r.txt", 50.0)


# ---- the definition on a hand-made case ----------------------------------------------------------------------------
def test_the_order_of_two_overlapping_rules_decides():
    g = SM.latlon_grid(4, 10, lon0=0.0, lat0=0.0, dlon=1.0, dlat=1.0)   # centres at 0.5 .. 9.5 x 0.5 .. 3.5
    wet = np.ones((4, 10), np.uint8)
    wet[:, 7] = 0   # a wall: the columns 8 and 9 belong to nobody's seed
    a = (1, 0.5, 0.5, 0.0, 6.0, 0.0, 4.0)     # columns 0 .. 5
    b = (2, 9.5, 0.5, 3.0, 10.0, 0.0, 4.0)    # columns 3 .. 9, seeded behind the wall
    c = (3, 4.5, 0.5, 3.0, 10.0, 0.0, 4.0)    # columns 3 .. 9, seeded in the overlap
    code, rule_, rec = D.basin_codes(g["x"], g["y"], wet, [a, c], False, False)
    assert np.all(code[:, :6] == 1) and np.all(code[:, 6:] == 0)   # c's seed cell is a's: c takes nothing
    assert rec["status"].tolist() == [D.TOOK, D.SEED_CODED] and rec["blocking_rule"].tolist() == [-1, 0] and rec["cells"].tolist() == [24, 0]
    code2, rule2, rec2 = D.basin_codes(g["x"], g["y"], wet, [c, a], False, False)
    assert np.all(code2[:, :3] == 1) and np.all(code2[:, 3:7] == 3) and np.all(code2[:, 7:] == 0)
    assert rec2["cells"].tolist() == [16, 12] and rec2["status"].tolist() == [D.TOOK, D.TOOK]
    assert not np.array_equal(code, code2)
    assert np.array_equal(rule2 == 0, code2 == 3) and np.array_equal(rule2 == -1, code2 == 0)
    # a rule seeded behind the wall takes only what it reaches; seeded on the wall it reports land
    code3, _, rec3 = D.basin_codes(g["x"], g["y"], wet, [a, b, (4, 7.5, 2.5, 0.0, 10.0, 0.0, 4.0)], False, False)
    assert np.all(code3[:, 8:] == 2) and np.all(code3[:, 6] == 0) and rec3["status"].tolist() == [D.TOOK, D.TOOK, D.SEED_LAND]
    assert rec3["seed_cell"].tolist() == [0, 9, 27]
