"""The device sill depths held EQUAL to the definition of tests/sill_definition.py: b, region, gate_u, gate_v and every count, no
tolerance.  The planes are the smallest that cross what the kernels can get wrong: one cell, one row, two vertical tile edges (130
columns), two tile rows at the default height (70 rows), 65 x 129 with both, and 33 x 64, whose fold's middle pair lies on no tile edge
while 3 x 130's lies next to one; every plane under all four topologies; ties, land, extremes, clamped weights; several seed patterns;
a serpentine channel about 2000 passages long; tile heights; poison in the faces that are never read."""
import os

import numpy as np
import pytest

import sill_definition as D

pytestmark = pytest.mark.gpu
PLANES = [(1, 1), (1, 2), (2, 2), (1, 130), (3, 130), (70, 3), (65, 129), (33, 64)]
KINDS = ["uniform", "three", "cells", "zero", "full", "clamped"]
BITS_OF = {(1, 1): 1, (1, 2): 2, (2, 2): 30, (1, 130): 21, (3, 130): 2, (70, 3): 30, (65, 129): 21, (33, 64): 1}
POISON = -0x7A7A7A7A


@pytest.fixture(scope="module")
def S(hip):
    from ocean_model_grid_generator_amd import sill_depth
    return sill_depth


def weights(kind, ny, nx, topology, bits, rng):
    top = (1 << bits) - 1
    shape_u, shape_v = (ny, nx + 1), (ny + 1, nx)
    if kind == "uniform":
        return rng.integers(0, top + 1, shape_u), rng.integers(0, top + 1, shape_v)
    if kind == "three":
        vals = np.array([0, max(top // 2, 1), top])
        return vals[rng.integers(0, 3, shape_u)], vals[rng.integers(0, 3, shape_v)]
    if kind == "cells":
        q = rng.integers(1, top + 1, (ny, nx))
        return D.cell_weights(q, rng.random((ny, nx)) >= 0.3, topology)
    if kind == "zero":
        return np.zeros(shape_u, np.int64), np.zeros(shape_v, np.int64)
    if kind == "full":
        return np.full(shape_u, top), np.full(shape_v, top)
    wu, wv = rng.integers(-top - 5, 2 * top + 5, shape_u), rng.integers(-top - 5, 2 * top + 5, shape_v)   # "clamped"
    return wu, wv


def check(S, wu, wv, seeds, topology, bits, dev=False):
    want = D.sill(wu, wv, seeds, topology, bits)
    if dev:
        import torch
        r = S.sill_depth_faces_dev(torch.from_numpy(np.asarray(wu)).cuda(), torch.from_numpy(np.asarray(wv)).cuda(), list(seeds),
                                   bool(topology & 1), bool(topology & 2), bits)
        got = {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in r.items()}
    else:
        got = S.sill_depth_faces(wu, wv, seeds, bool(topology & 1), bool(topology & 2), bits)
    for k in ("b", "region", "gate_u", "gate_v"):
        bad = np.argwhere(got[k] != want[k])
        assert bad.size == 0, (k, len(bad), bad[:5].tolist(), [(int(got[k][tuple(t)]), int(want[k][tuple(t)])) for t in bad[:5]])
    assert got["counts"] == want["counts"]
    return got


@pytest.mark.parametrize("topology", [0, 1, 2, 3])
@pytest.mark.parametrize("ny, nx", PLANES)
def test_planes_and_weights(S, ny, nx, topology):
    rng = np.random.default_rng(1000 * ny + 10 * nx + topology)
    bits = BITS_OF[(ny, nx)]
    for k, kind in enumerate(KINDS):
        wu, wv = weights(kind, ny, nx, topology, bits, rng)
        seeds = [int(rng.integers(0, ny * nx))]
        got = check(S, wu, wv, seeds, topology, bits, dev=k % 2 == 1)
        if kind == "clamped" and ny * nx > 4:
            assert got["counts"]["n_clamped"] > 0
        if kind == "zero":
            assert got["counts"]["n_connected"] == 0 and got["counts"]["n_cut_off"] == 0
        if kind == "full":
            assert got["counts"]["n_connected"] == ny * nx - 1


@pytest.mark.parametrize("bits", [1, 2, 21, 30])
@pytest.mark.parametrize("topology", [0, 3])
def test_every_bits(S, bits, topology):
    rng = np.random.default_rng(bits)
    for kind in ("uniform", "three", "cells"):
        wu, wv = weights(kind, 37, 67, topology, bits, rng)
        check(S, wu, wv, [5], topology, bits)


def test_bits_21_and_30_give_the_same_b(S):
    rng = np.random.default_rng(21)
    wu, wv = weights("cells", 40, 70, 3, 21, rng)
    a = check(S, wu, wv, [123], 3, 21)
    b = check(S, wu, wv, [123], 3, 30)
    assert a["b"].tobytes() == b["b"].tobytes() and a["region"].tobytes() == b["region"].tobytes()
    assert a["counts"]["rounds"] == 21 and b["counts"]["rounds"] == 30
    assert S.sill_depth_faces(wu, wv, [123], True, True)["bits"] == D.bits_for(wu, wv)


SEEDS = {"one": [700], "three": [3, 1400, 2600], "adjacent": [700, 701], "duplicated": [700, 700, 9, 700], "out_of_range": [700, 40 * 70],
         "negative": [-1, 700], "isolated": None}


@pytest.mark.parametrize("name", sorted(SEEDS))
@pytest.mark.parametrize("topology", [0, 3])
def test_seeds(S, name, topology):
    ny, nx = 40, 70
    rng = np.random.default_rng(7)
    wu, wv = weights("three" if name == "adjacent" else "cells", ny, nx, topology, 12, rng)
    seeds = SEEDS[name]
    if seeds is None:   # a cell all of whose faces are closed
        j, i = 20, 30
        wu[j, i] = wu[j, i + 1] = wv[j, i] = wv[j + 1, i] = 0
        seeds = [j * nx + i]
    got = check(S, wu, wv, seeds, topology, 12)
    if name in ("out_of_range", "negative"):
        assert got["counts"]["n_bad_seeds"] == 1
    if name == "isolated":
        assert got["counts"]["n_connected"] == 0 and got["counts"]["n_cut_off"] > 0


@pytest.mark.parametrize("shallow", [None, 1100])
def test_serpentine(S, shallow):
    wu, wv, seed, m = D.serpentine(64, 66, shallow)
    assert m > 2000
    got = check(S, wu, wv, [seed], 0, None)
    assert got["counts"]["n_connected"] == m
    levels = np.unique(got["b"][(got["b"] > 0) & (got["b"] < D.SEED)])
    assert levels.size == (m if shallow is None else shallow + 1)
    assert got["counts"]["n_regions"] == levels.size + 1


def test_tile_rows_give_the_same_bytes(S, monkeypatch):
    rng = np.random.default_rng(3)
    wu, wv = weights("three", 70, 131, 3, 9, rng)
    out = []
    for th in ("8", "32", "64"):
        monkeypatch.setenv("OGG_SILL_TILE_ROWS", th)
        got = check(S, wu, wv, [4000, 17], 3, 9, dev=th == "32")
        out.append(b"".join(got[k].tobytes() for k in ("b", "region", "gate_u", "gate_v")))
    assert out[0] == out[1] == out[2]
    monkeypatch.setenv("OGG_SILL_TILE_ROWS", "65")
    with pytest.raises(Exception, match="OGG_SILL_TILE_ROWS"):
        S.sill_depth_faces(wu, wv, [1], True, True, 9)


@pytest.mark.parametrize("topology", [0, 1, 2, 3])
@pytest.mark.parametrize("ny, nx", [(5, 7), (4, 2), (3, 1), (33, 64)])
def test_poison_in_the_faces_never_read(S, ny, nx, topology):
    rng = np.random.default_rng(ny + nx)
    wu, wv = weights("uniform", ny, nx, topology, 10, rng)
    a = check(S, wu, wv, [0], topology, 10)
    pu, pv = wu.copy(), wv.copy()
    pv[0] = POISON
    if not (topology & 1) or nx <= 2:
        pu[:, 0] = pu[:, nx] = POISON
    if not (topology & 2):
        pv[ny] = POISON
    elif nx % 2:
        pv[ny, nx // 2] = POISON
    b = S.sill_depth_faces(pu, pv, [0], bool(topology & 1), bool(topology & 2), 10)
    for k in ("b", "region", "gate_u", "gate_v"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert a["counts"] == b["counts"]


def test_argument_errors(S):
    wu, wv = np.zeros((3, 5), np.int64), np.zeros((4, 4), np.int64)
    with pytest.raises(ValueError, match="bits"):
        S.sill_depth_faces(wu, wv, [0], False, False, 31)
    with pytest.raises(ValueError, match="at least one seed"):
        S.sill_depth_faces(wu, wv, [], False, False, 4)
    with pytest.raises(ValueError, match="integer"):
        S.sill_depth_faces(wu.astype(float), wv, [0], False, False, 4)
    with pytest.raises(ValueError, match="must be"):
        S.sill_depth_faces(wu, wv[:3], [0], False, False, 4)


# ---- depths, both weight modes, host and device ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def raster_case(hip):
    import small_grids as G
    from ocean_model_grid_generator_amd import face_topography as FT
    from ocean_model_grid_generator_amd import topography as T
    x, y = G.grid(24, 40, lon0=104.0, lat0=-4.0, d=0.5)
    r = G.raster("float32_q0.01")
    src = T.Source(r["data"], *r["box"], fill=r["fill"], quantum=r["quantum"])
    topo = T.topography(x, y, src)
    faces = FT.face_topography(x, y, src)
    return x, y, topo["depth"], faces


@pytest.mark.parametrize("mode", ["cells", "faces"])
def test_dev_equals_host_and_the_definition(S, raster_case, mode):
    import torch
    x, y, depth, faces = raster_case
    ny, nx = depth.shape
    host = S.sill_depth(depth, x, y, faces=faces, weights=mode, quantum=0.01, min_cells=2)
    dev = S.sill_depth_dev(torch.from_numpy(depth).cuda(), torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), faces=faces,
                           weights=mode, quantum=0.01, min_cells=2)
    for k in ("sill_depth", "reach", "region", "gate_u", "gate_v", "b"):
        assert host[k].dtype == dev[k].dtype and host[k].tobytes() == dev[k].tobytes(), k
    assert host["counts"] == dev["counts"] and host["basins"] == dev["basins"] and host["summary"] == dev["summary"]
    q = D.quantise(depth, 0.01)
    wet = q > 0
    assert wet.any() and host["summary"]["seeds"][0]["cell"] == int(np.argmax(q.reshape(-1)))
    if mode == "cells":
        wu, wv = D.cell_weights(q, wet, 0)
    else:
        ou, ov = D.cell_weights(wet.astype(np.int64), wet, 0)
        wu, wv = D.quantise(faces["u"]["depth_max"], 0.01) * ou, D.quantise(faces["v"]["depth_max"], 0.01) * ov
    want = D.sill(wu, wv, [host["summary"]["seeds"][0]["cell"]], 0)
    for k in ("b", "region", "gate_u", "gate_v"):
        assert np.array_equal(host[k], want[k]), k
    assert host["counts"] == want["counts"]
    b = host["b"]
    assert np.array_equal(host["reach"], np.where(b == D.SEED, 2, np.where(b > 0, 1, np.where(wet, 3, 0))))
    seed = np.unravel_index(host["summary"]["seeds"][0]["cell"], b.shape)
    assert host["sill_depth"][seed] == q[seed] * 0.01 and np.all(host["sill_depth"][b == 0] == 1.0e20)
    for k in host["basins"]:
        assert k["cells"] >= 2 and k["cells"] == int(np.sum(host["region"] == k["region"])) and k["n_gates"] >= 1
        assert k["sill_depth"] == float(b.reshape(-1)[k["region"]] * 0.01)
