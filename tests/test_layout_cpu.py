"""CPU tests of the processor layouts and mask tables (csrc/ogg_layout.hip's host side, layout.py): ogg_layout_extent against the
definition of tests/layout_definition.py and the known answers of the header's rule, the checks before any device work, the
workspace size, the branches of the definition's own neighbourhood on hand-made inputs, the table text, the flag validation and the
ranking's ties.  No device call is made here."""
import ctypes

import numpy as np
import pytest

import layout_definition as D


@pytest.fixture(scope="module")
def LY():
    from ocean_model_grid_generator_amd import layout as m
    return m


@pytest.fixture(scope="module")
def L():
    from ocean_model_grid_generator_amd import _lib
    _lib.load()
    return _lib


def sizes(LY, npts, ndivs):
    b, e = LY.extent(npts, ndivs)
    return (e - b + 1).tolist()


# ---- the extent rule ------------------------------------------------------------------------------------------------
def test_extent_equals_the_definition(LY):
    for npts in range(1, 201):
        for ndivs in range(1, npts + 1):
            b, e = LY.extent(npts, ndivs)
            assert (b.tolist(), e.tolist()) == D.extent(npts, ndivs), (npts, ndivs)


KNOWN = [(10, 4, [3, 2, 2, 3], True), (10, 3, [4, 2, 4], True), (11, 4, [3, 3, 3, 2], False), (12, 5, [3, 2, 2, 2, 3], True),
         (8, 3, [3, 2, 3], True), (6, 3, [2, 2, 2], False), (5, 4, [2, 1, 1, 1], False),
         (2880, 7, [412, 412, 411, 410, 411, 412, 412], True), (1440, 36, [40] * 36, True)]


@pytest.mark.parametrize("npts, ndivs, want, sym", KNOWN)
def test_extent_known_answers(LY, npts, ndivs, want, sym):
    assert sizes(LY, npts, ndivs) == want and D.is_symmetric(npts, ndivs) == sym
    assert [e - b + 1 for b, e in zip(*D.extent(npts, ndivs))] == want


def test_extent_1080_by_32(LY):
    s = sizes(LY, 1080, 32)
    assert sorted(set(s)) == [33, 34] and sum(s) == 1080 and s == s[::-1] and D.is_symmetric(1080, 32)


def test_extent_is_a_partition_and_symmetric_where_the_rule_says_so(LY):
    cases = [(n, d) for n in range(1, 201) for d in range(1, n + 1)]
    rng = np.random.default_rng(5)
    cases += [(int(n), int(rng.integers(1, min(n, 4096) + 1))) for n in rng.integers(1, 2**31 - 1, 300)]
    for npts, ndivs in cases:
        b, e = LY.extent(npts, ndivs)
        assert b[0] == 0 and e[-1] == npts - 1 and np.all(e >= b) and np.all(b[1:] == e[:-1] + 1), (npts, ndivs)
        s = e.astype(np.int64) - b + 1
        assert s.max() - s.min() <= 2, (npts, ndivs)
        if D.is_symmetric(npts, ndivs):
            assert np.array_equal(s, s[::-1]), (npts, ndivs)


def test_extent_refuses_bad_sizes(LY, L):
    for npts, ndivs in ((0, 1), (5, 0), (5, 6), (-3, 1), (2**31, 1)):
        with pytest.raises(ValueError, match="ogg_layout_extent"):
            LY.extent(npts, ndivs)
    assert L.load().ogg_layout_extent(4, 2, None, None) == L.OGG_EARG
    b = np.empty(2, np.int32)
    assert L.load().ogg_layout_extent(4, 2, b.ctypes.data, None) == L.OGG_OK and b.tolist() == [0, 2]   # end may be NULL


# ---- the checks and the workspace -------------------------------------------------------------------------------------
def test_check_refuses_bad_sizes_halo_and_zero_divisions(LY, L):
    LY.params(5, 7, True, True, 3)
    for ny, nx in ((0, 5), (5, 0), (-1, 5), (1 << 16, 1 << 15), (1 << 31, 1)):
        with pytest.raises(ValueError, match="ny, nx >= 1 and ny \\* nx < 2\\^31"):
            LY.params(ny, nx)
    LY.params((1 << 16) - 1, 1 << 15)
    with pytest.raises(ValueError, match="halo -1"):
        LY.params(5, 7, halo=-1)
    p = L.LayoutParams(ny=5, nx=7, topology=4, halo=0)
    assert L.load().ogg_layout_check(ctypes.byref(p), None, 0) == L.OGG_EARG and b"topology" in L.load().ogg_last_error()
    assert L.load().ogg_layout_check(None, None, 0) == L.OGG_EARG
    for bad in ((0, 2), (2, 0), (-1, 1)):
        with pytest.raises(ValueError, match="candidate 1 is %d x %d" % bad):
            LY.params(5, 7, candidates=LY.as_candidates([(1, 1), bad]))
    LY.params(5, 7, candidates=LY.as_candidates([(1, 1), (8, 6), (5000, 1)]))   # finer than the grid: a status, no refusal
    p = LY.params(5, 7)
    assert L.load().ogg_layout_check(ctypes.byref(p), None, 1) == L.OGG_EARG
    assert L.load().ogg_layout_check(ctypes.byref(p), None, L.LAYOUT_MAX_CANDIDATES + 1) == L.OGG_EARG


def test_workspace_is_positive_and_monotone(LY, L):
    lib = L.load()
    size = lambda ny, nx: int(lib.ogg_layout_workspace_bytes(ctypes.byref(L.LayoutParams(ny=ny, nx=nx, topology=0, halo=0))))   # noqa: E731
    assert lib.ogg_layout_workspace_bytes(None) == -1 and size(0, 4) == -1
    prev = 0
    for n in (1, 2, 7, 64, 65, 300, 1080, 2240):
        s = size(n, n + 3)
        assert s >= (n + 1) * (n + 4) * 4 and s >= prev > -1   # monotone: the sections are rounded up, so small sizes may tie
        assert size(n + 1, n + 3) >= s and size(n, n + 4) >= s
        prev = s
    assert size(2240, 2880) > size(1080, 1440) > size(64, 65) > 0


# ---- the definition's own branches --------------------------------------------------------------------------------------
def test_definition_halo_across_the_seam():
    # 3 x 8 cells, the block of columns 0 .. 1: a halo of 1 reaches column 7 only on a periodic grid
    assert D.neighbourhood(3, 8, True, False, 1, 1, 1, 0, 1) == {(j, i) for j in (0, 1, 2) for i in (7, 0, 1, 2)}
    assert D.neighbourhood(3, 8, False, False, 1, 1, 1, 0, 1) == {(j, i) for j in (0, 1, 2) for i in (0, 1, 2)}
    wet = np.zeros((3, 8), np.uint8)
    wet[1, 7] = 1
    own, nbr, _ = D.blocks(wet, 4, 1, True, False, 1)
    assert own.tolist() == [[0, 0, 0, 1]] and nbr.tolist() == [[1, 0, 0, 1]]
    assert D.blocks(wet, 4, 1, False, False, 1)[1].tolist() == [[0, 0, 0, 1]]


def test_definition_halo_across_the_fold_onto_mirrored_columns():
    # 4 x 10 cells, the block of rows 2 .. 3 and columns 1 .. 2: row 4 is row 3 at the mirrored columns 9 - (0 .. 3) = 6 .. 9
    got = D.neighbourhood(4, 10, True, True, 1, 2, 3, 1, 2)
    assert got == {(j, i) for j in (1, 2, 3) for i in (0, 1, 2, 3)} | {(3, i) for i in (6, 7, 8, 9)}
    assert D.neighbourhood(4, 10, True, False, 1, 2, 3, 1, 2) == {(j, i) for j in (1, 2, 3) for i in (0, 1, 2, 3)}
    wet = np.zeros((4, 10), np.uint8)
    wet[3, 8] = 1
    assert D.blocks(wet, 5, 2, True, True, 1)[1].tolist() == [[0, 0, 0, 0, 0], [1, 1, 0, 1, 1]]   # blocks 0 and 1 across the fold
    assert D.blocks(wet, 5, 2, True, False, 1)[1].tolist() == [[0, 0, 0, 0, 0], [0, 0, 0, 1, 1]]
    # a column past the seam wraps first and is mirrored then: column -1 -> 9 -> 0
    assert (3, 0) in D.neighbourhood(4, 10, True, True, 1, 3, 3, 0, 0) and (3, 8) in D.neighbourhood(4, 10, True, True, 1, 3, 3, 0, 0)


def test_definition_halo_as_wide_as_the_grid():
    every = {(j, i) for j in range(3) for i in range(5)}
    assert D.neighbourhood(3, 5, True, True, 13, 1, 1, 2, 2) == every and D.neighbourhood(3, 5, True, False, 5, 0, 0, 0, 0) == every
    assert D.neighbourhood(3, 5, False, False, 13, 1, 1, 2, 2) == every
    # rows past the fold by the grid's height or more are dropped: k = 3 maps nowhere
    assert D.neighbourhood(3, 5, False, True, 2, 2, 2, 0, 0) == {(j, i) for j in range(3) for i in (0, 1, 2)} | {(j, i) for j in (1, 2) for i in (2, 3, 4)}
    wet = np.ones((3, 5), np.uint8)
    own, nbr, _ = D.blocks(wet, 5, 3, True, True, 13)
    assert np.all(own == 1) and np.all(nbr == 15)   # each cell once, however often the halo reaches it


def test_definition_array_form_is_the_set_form():
    """reached() (what the GPU tests count with) marks exactly the cells of neighbourhood()"""
    rng = np.random.default_rng(3)
    for _ in range(300):
        ny, nx = int(rng.integers(1, 9)), int(rng.integers(1, 12))
        by, bx = int(rng.integers(0, ny)), int(rng.integers(0, nx))
        ey, ex = int(rng.integers(by, ny)), int(rng.integers(bx, nx))
        periodic, fold, h = bool(rng.integers(2)), bool(rng.integers(2)), int(rng.choice([0, 1, 2, 3, 13, 30]))
        got = D.reached(ny, nx, periodic, fold, h, by, ey, bx, ex)
        assert {(int(j), int(i)) for j, i in zip(*np.nonzero(got))} == D.neighbourhood(ny, nx, periodic, fold, h, by, ey, bx, ex)


def test_definition_fold_without_a_seam():
    # the columns outside the grid are dropped before the mirror: block of columns 0 .. 1 on the top row, halo 1
    got = D.neighbourhood(2, 6, False, True, 1, 1, 1, 0, 1)
    assert got == {(j, i) for j in (0, 1) for i in (0, 1, 2)} | {(1, i) for i in (3, 4, 5)}
    rec = D.record(np.ones((2, 7), np.uint8), 4, 1, False, True, 0)   # 7 columns four ways: 2, 2, 2, 1
    assert rec["status"] == D.FOLD_ASYMMETRIC and rec["min_block_size"] == 1 and rec["max_block_cells"] == 4
    assert D.record(np.ones((2, 7), np.uint8), 4, 1, False, False, 0)["status"] == 0
    assert D.record(np.ones((2, 7), np.uint8), 3, 1, False, True, 0)["status"] == 0
    assert D.record(np.ones((2, 7), np.uint8), 8, 1, False, True, 0) == dict({f: 0 for f in D.FIELDS}, status=D.TOO_FINE)


# ---- the table's text ---------------------------------------------------------------------------------------------------
def test_mask_table_round_trip_and_exact_bytes(LY, tmp_path):
    masked = [(2, 0), (0, 1)]   # ascending (b, a)
    path = LY.write_mask_table(str(tmp_path), 3, 2, masked)
    assert path == str(tmp_path / "mask_table.2.3x2")
    assert open(path, "rb").read() == b"2\n3,2\n3,1\n1,2\n" == D.table_text(3, 2, masked).encode()
    px, py, got = LY.read_mask_table(path)
    assert (px, py) == (3, 2) and got.tolist() == [[2, 0], [0, 1]] and got.dtype == np.int32
    named = LY.write_mask_table(str(tmp_path / "mine.txt"), {"px": 3, "py": 2, "masked": np.array(masked, np.int32)})
    assert open(named, "rb").read() == open(path, "rb").read()
    empty = LY.write_mask_table(str(tmp_path), 4, 4, [])
    assert empty.endswith("mask_table.0.4x4") and open(empty).read() == "0\n4,4\n" and LY.read_mask_table(empty)[2].shape == (0, 2)
    for text in ("", "1\n3,2\n", "1\n3,2\n4,1\n", "x\n3,2\n"):
        open(str(tmp_path / "bad"), "w").write(text)
        with pytest.raises(ValueError, match="bad"):
            LY.read_mask_table(str(tmp_path / "bad"))


# ---- the flags ----------------------------------------------------------------------------------------------------------
def test_flag_validation_texts():
    from ocean_model_grid_generator_amd import ocean_grid_generator as ogg
    check = lambda **f: ogg._validate_all((), 0.0, -99.0, f.pop("skip_metrics", False), ogg.AnalysisFlags(**f))   # noqa: E731
    a = ogg.AnalysisFlags()
    assert a.mask_table_layout is None and a.layout_sweep is None and a.layout_halo == 0 and a.layout_min_block == 2
    check()
    check(topog_source="t.nc", mask_table_layout=[(3, 2)], skip_metrics=True)
    check(topog_source="t.nc", layout_sweep=64, layout_target_pes=40, layout_halo=2, layout_min_block=1, layout_report="l.json")
    check(topog_source="t.nc", mask_table_layout=[(3, 2)], layout_xextent="3,3,4", layout_yextent="5,5")
    for flags, text in (
            (dict(mask_table_layout=[(3, 2)]), "--mask_table_layout and --layout_sweep need --topog_source"),
            (dict(layout_sweep=64), "--mask_table_layout and --layout_sweep need --topog_source"),
            (dict(layout_target_pes=8), "need --mask_table_layout or --layout_sweep"),
            (dict(topog_source="t.nc", layout_halo=1), "need --mask_table_layout or --layout_sweep"),
            (dict(topog_source="t.nc", mask_table_dir="d"), "need --mask_table_layout or --layout_sweep"),
            (dict(topog_source="t.nc", layout_sweep=64, layout_halo=-1), "--layout_halo must be >= 0, not -1"),
            (dict(topog_source="t.nc", layout_sweep=64, layout_min_block=0), "--layout_min_block must be >= 1, not 0"),
            (dict(topog_source="t.nc", layout_sweep=0), "--layout_sweep must be >= 1 block, not 0"),
            (dict(topog_source="t.nc", mask_table_layout=[(3, 2)], layout_target_pes=4), "--layout_target_pes needs --layout_sweep"),
            (dict(topog_source="t.nc", layout_sweep=64, layout_target_pes=0), "--layout_target_pes must be >= 1, not 0"),
            (dict(topog_source="t.nc", mask_table_layout=[(0, 2)]), "--mask_table_layout takes PX PY, both >= 1"),
            (dict(topog_source="t.nc", layout_sweep=64, layout_xextent="3,3"), "need exactly one --mask_table_layout"),
            (dict(topog_source="t.nc", mask_table_layout=[(3, 2), (2, 2)], layout_yextent="3,3"), "need exactly one --mask_table_layout"),
            (dict(topog_source="t.nc", mask_table_layout=[(3, 2)], layout_xextent="3,a"), "--layout_xextent takes a comma list of block sizes")):
        with pytest.raises(ValueError, match=text):
            check(**flags)
    a = ogg.build_parser().parse_args(["-r", "4", "--mask_table_layout", "3", "2", "--mask_table_layout", "4", "4", "--layout_sweep", "64"])
    assert a.mask_table_layout == [[3, 2], [4, 4]] and a.layout_sweep == 64 and a.layout_halo == 0 and a.layout_min_block == 2


def test_explicit_extents_are_checked(LY):
    assert LY._begins([3, 3, 4], 10, 3, "xextent").tolist() == [0, 3, 6] and LY._begins(None, 10, 3, "xextent") is None
    for bad in ([3, 3, 3], [5, 5], [10, 0, 0], [11, -1, 0]):
        with pytest.raises(ValueError, match="xextent holds"):
            LY._begins(bad, 10, 3, "xextent")


# ---- the ranking --------------------------------------------------------------------------------------------------------
def test_best_layouts_resolves_ties_by_the_stated_key(LY):
    rows = [  # px, py, blocks, masked, pes, cells, edge, min, max_wet, masked_cells, wet_total, status
        (4, 3, 12, 2, 10, 100, 20, 5, 9, 0, 50, 0),
        (3, 4, 12, 2, 10, 100, 20, 5, 9, 0, 50, 0),    # the same key up to px: the smaller px wins
        (2, 6, 12, 2, 10, 100, 21, 5, 9, 0, 50, 0),    # a longer edge loses
        (5, 2, 10, 0, 10, 100, 20, 5, 9, 0, 50, 0),    # fewer blocks win over (3, 4)
        (1, 10, 10, 0, 10, 90, 91, 1, 9, 0, 50, 2),    # smaller blocks, but refused by its status
        (10, 1, 10, 0, 10, 101, 11, 1, 9, 0, 50, 0),   # larger blocks lose whatever the edge
        (3, 3, 9, 0, 9, 120, 22, 5, 9, 0, 50, 0),
        (9, 1, 9, 1, 8, 130, 22, 5, 9, 0, 50, 0),
        (4, 4, 16, 5, 11, 80, 18, 5, 9, 0, 50, 0)]     # above the target: no near miss
    rec = np.array(rows, dtype=LY.RECORD)
    got = LY.best_layouts(rec, 10)
    assert (got["best"]["px"], got["best"]["py"]) == (5, 2) and [(r["px"], r["py"], r["pes"]) for r in got["by_pes"]] == [(5, 2, 10), (3, 3, 9), (9, 1, 8)]
    assert (LY.best_layouts(rec[:3], 10)["best"]["px"], LY.best_layouts(rec[[0, 1]][::-1], 10)["best"]["px"]) == (3, 3)
    assert LY.best_layouts(rec, 7) == {"target_pes": 7, "best": None, "by_pes": []}
    assert LY.best_layouts(rec, 12)["best"] is None and LY.best_layouts(rec, 12)["by_pes"][0]["pes"] == 11
    want, by = D.best([LY.record_dict(r) for r in rec], 10)
    assert got["best"] == want and got["by_pes"] == [by[k] for k in sorted(by, reverse=True)]
    with pytest.raises(ValueError, match="target"):
        LY.best_layouts(rec, 0)


def test_sweep_candidates_follow_the_extents(LY):
    c = LY.sweep_candidates(9, 12, 20, 2)
    want = [(px, py) for px in range(1, 13) for py in range(1, 10)
            if px * py <= 20 and min(e - b + 1 for ax, d in ((12, px), (9, py)) for b, e in zip(*D.extent(ax, d))) >= 2]
    assert list(zip(c["px"].tolist(), c["py"].tolist())) == want and (6, 3) in want and (5, 1) in want and (1, 5) not in want
    assert LY.sweep_candidates(9, 12, 1000, 1).shape[0] == 9 * 12 and LY.sweep_candidates(1, 1, 5).shape[0] == 0
    assert LY.sweep_candidates(3, 5000, 10**6, 1)["px"].max() == 4096
