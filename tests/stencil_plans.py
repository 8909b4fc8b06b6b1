"""The settings that reach every instantiation of the generic stencil kernel at small shapes (used by tests/test_stencil_bounds_cpu.py, which
asserts the coverage without a GPU, and by the GPU tests, which assert the same plan through ogg_grid_metrics_midas_plan before they launch).

ogg_grid_metrics_midas_dev walks rpb = ceil(n_pt_rows * column tiles / OGG_MIDAS_TARGET_WG) point rows per workgroup: held to 2 ..
min(OGG_MIDAS_TILE_ROWS, 12) and to n_pt_rows for the LDS-staged tile kernel, whose instantiation TR is the smallest of 4, 6, 8, 12 that holds rpb, and to
4 (1 for an angle-only call) .. 16 for the streaming kernel (OGG_MIDAS_TILE_ROWS=0).  With the default target of 2048 workgroups every mesh of a
few thousand points gets the minimum; OGG_MIDAS_TARGET_WG=1 asks for one workgroup per column tile, so the tile height is what
OGG_MIDAS_TILE_ROWS says.
"""
import ctypes
import os

TX = 256                       # columns per workgroup
TILE_ROWS_MAX, STREAM_ROWS_MAX = 12, 16
TILE_SETTINGS = tuple(range(1, 13)) + (99,)


def expected(ni1, n_pt_rows, metrics, tile_rows, target):
    """(TR or 0, rows per block) as csrc/ogg_midas.hip plans it."""
    gx = (ni1 + TX - 1) // TX
    rpb = (n_pt_rows * gx + target - 1) // target
    if tile_rows > 0:
        rpb = min(2 if rpb < 2 else min(rpb, tile_rows), TILE_ROWS_MAX, n_pt_rows)      # the floor of 2 is not cut by a setting of 1
        return (4 if rpb <= 4 else 6 if rpb <= 6 else 8 if rpb <= 8 else 12), rpb
    return 0, min(max(rpb, 4 if metrics else 1), STREAM_ROWS_MAX)


def variants(ni1, n_pt_rows, metrics):
    """[(label, {environment}, (TR or 0, rows per block))]: every tile setting at one workgroup per column tile, and the streaming kernel at
    its smallest height, at 4 rows and at its largest height the mesh allows."""
    gx = (ni1 + TX - 1) // TX
    out = []
    for k in TILE_SETTINGS:
        out.append(("tile%d" % k, {"OGG_MIDAS_TILE_ROWS": str(k), "OGG_MIDAS_TARGET_WG": "1"}, expected(ni1, n_pt_rows, metrics, k, 1)))
    for label, target in (("stream_min", 2048), ("stream4", -(-(n_pt_rows * gx) // 4)), ("stream_max", 1)):
        out.append((label, {"OGG_MIDAS_TILE_ROWS": "0", "OGG_MIDAS_TARGET_WG": str(target)}, expected(ni1, n_pt_rows, metrics, 0, target)))
    return out


def planned(lib, ni1, n_pt_rows, metrics, env=None, setenv=None):
    """(TR or 0, rows per block) from the library's own query under `env` (set through `setenv(name, value)`, e.g. monkeypatch.setenv; the
    process environment is restored by the caller's fixture, or here when setenv is None)."""
    env = env or {}
    old = {k: os.environ.get(k) for k in env}
    try:
        for k, v in env.items():
            (setenv or os.environ.__setitem__)(k, v)
        tr, rpb = ctypes.c_int(-1), ctypes.c_int(-1)
        lib.call("ogg_grid_metrics_midas_plan", ni1, n_pt_rows, int(bool(metrics)), ctypes.byref(tr), ctypes.byref(rpb))
        return tr.value, rpb.value
    finally:
        if setenv is None:
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
