"""Processor layouts and mask tables: for a decomposition of the model cells into px x py blocks (MOM6's LAYOUT = px,py) the blocks
that hold no ocean, which a run leaves without a process (MASKTABLE = mask_table.<n>.<px>x<py>), and over many candidate layouts
the ones that reach a given process count after masking, ranked by block size.  include/ogg_hip.h, "Processor layouts and mask
tables", gives the definition; the reference has no such step.

The wet set's summed-area table and the records of all candidates come from the device (ogg_layout_table_dev, ogg_layout_sweep_dev,
ogg_layout_blocks_dev, or the host-pointer ogg_layouts); the ranking and the table text are host code over those integers, so every
path, knob and rank count writes the same bytes.  CAVEAT: the extents follow FMS's mpp_compute_extent as restated in the header; no
copy of FMS or FRE-NCtools was on hand to verify the restatement, so ``xextent`` / ``yextent`` (block sizes, as FMS's own xextent and
yextent) tie a table to a model's own decomposition.

    python -m ocean_model_grid_generator_amd.layout (--topog topog.nc | --mask ocean_mask.nc) (--grid ocean_hgrid.nc | [--periodic]
        [--fold]) [--mask_table_layout PX PY]... [--layout_sweep MAX_BLOCKS] [--layout_target_pes T] [--mask_table_dir DIR]
        [--layout_report layouts.json] [--layout_halo H] [--layout_min_block N] [--layout_xextent a,b,..] [--layout_yextent a,b,..]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

from . import _lib as L
from . import fields as F

# a candidate's px, py in front of its ogg_layout_record
RECORD = np.dtype([("px", "<i4"), ("py", "<i4")] + [(f, "<i4") for f in L.LAYOUT_RECORD_FIELDS])
FLAG_DEFAULTS = dict(mask_table_layout=None, mask_table_dir=None, layout_sweep=None, layout_target_pes=None, layout_report=None,
                     layout_halo=0, layout_min_block=2, layout_xextent=None, layout_yextent=None)


# ---- arguments -----------------------------------------------------------------------------------------------
def params(ny, nx, periodic=False, fold=False, halo=0, candidates=None):
    """an ogg_layout_params, checked by the library together with the candidates (OGG_EARG -> ValueError)"""
    from . import ocean_mask as M
    p = L.LayoutParams(ny=int(ny), nx=int(nx), topology=M.topology_flags(periodic, fold), halo=int(halo))
    n = 0 if candidates is None else len(candidates)
    return L.checked("ogg_layout_check", p, candidates.ctypes.data if n else None, n)


def extent(npts, ndivs):
    """(begin, end) int32 arrays of ogg_layout_extent: the blocks of 0 .. npts-1 divided ndivs ways"""
    begin, end = np.empty(max(int(ndivs), 0), np.int32), np.empty(max(int(ndivs), 0), np.int32)
    lib = L.load()
    if lib.ogg_layout_extent(int(npts), int(ndivs), begin.ctypes.data, end.ctypes.data) != L.OGG_OK:
        raise ValueError(lib.ogg_last_error().decode())
    return begin, end


def as_candidates(candidates):
    """(n, 2) pairs (px, py), or a record array with px and py, as ogg_layout_candidate records"""
    if isinstance(candidates, np.ndarray) and candidates.dtype.names:
        c = np.empty(candidates.shape[0], L.LAYOUT_CANDIDATE)
        c["px"], c["py"] = candidates["px"], candidates["py"]
        return c
    a = np.asarray(candidates, dtype=np.int64).reshape(-1, 2)
    if a.size and (a.min() < -2**31 or a.max() >= 2**31):
        raise ValueError("layouts: a candidate does not fit 32 bits")
    c = np.empty(a.shape[0], L.LAYOUT_CANDIDATE)
    c["px"], c["py"] = a[:, 0], a[:, 1]
    return c


def _min_sizes(npts, nmax):
    """m[d] = the smallest block of npts divided d ways, d = 1 .. nmax (m[0] = 0)"""
    m = np.zeros(nmax + 1, np.int64)
    for d in range(1, nmax + 1):
        b, e = extent(npts, d)
        m[d] = int((e - b).min()) + 1
    return m


def sweep_candidates(ny, nx, max_blocks, min_block=2):
    """every (px, py) with px * py <= max_blocks, px <= nx, py <= ny, both <= OGG_LAYOUT_MAX_DIV, whose smallest extent (by
    ogg_layout_extent) is at least min_block, as ogg_layout_candidate records in ascending (px, py)"""
    max_blocks, min_block = int(max_blocks), int(min_block)
    if max_blocks < 1 or min_block < 1:
        raise ValueError("layouts: max_blocks and min_block must be >= 1, not %d and %d" % (max_blocks, min_block))
    mx = _min_sizes(nx, min(nx, max_blocks, L.LAYOUT_MAX_DIV))
    my = _min_sizes(ny, min(ny, max_blocks, L.LAYOUT_MAX_DIV))
    out = []
    for px in range(1, mx.size):
        if mx[px] < min_block:
            continue
        py = np.arange(1, min(my.size - 1, max_blocks // px) + 1)
        py = py[my[py] >= min_block]
        out.append(np.stack([np.full(py.size, px), py], axis=1))
    c = as_candidates(np.concatenate(out) if out else np.zeros((0, 2), np.int64))
    if c.size > L.LAYOUT_MAX_CANDIDATES:
        raise ValueError("layouts: %d candidates, at most %d in one sweep" % (c.size, L.LAYOUT_MAX_CANDIDATES))
    return c


def _candidates_for(shape, candidates, max_blocks, min_block):
    if (candidates is None) == (max_blocks is None):
        raise ValueError("layouts: give either the candidates or max_blocks")
    return as_candidates(candidates) if candidates is not None else sweep_candidates(shape[0], shape[1], max_blocks, min_block)


def _begins(sizes, npts, ndivs, name):
    """None, or the begins of explicit block sizes (FMS's xextent / yextent) after their checks"""
    if sizes is None:
        return None
    s = np.asarray(sizes, dtype=np.int64).reshape(-1)
    if s.size != ndivs or (s < 1).any() or int(s.sum()) != npts:
        raise ValueError("mask table: %s holds %d sizes with sum %d: %d sizes >= 1 with sum %d are needed"
                         % (name, s.size, int(s.sum()), ndivs, npts))
    return np.ascontiguousarray(np.concatenate(([0], np.cumsum(s)[:-1])), dtype=np.int32)


def _joined(cand, rec):
    out = np.empty(cand.shape[0], RECORD)
    out["px"], out["py"] = cand["px"], cand["py"]
    for f in L.LAYOUT_RECORD_FIELDS:
        out[f] = rec[f]
    return out


def _sweep_result(records, shape, periodic, fold, halo, max_blocks, min_block):
    return {"records": records, "shape": [int(shape[0]), int(shape[1])], "periodic": bool(periodic), "fold": bool(fold), "halo": int(halo),
            "max_blocks": None if max_blocks is None else int(max_blocks), "min_block": int(min_block)}


def _table_result(px, py, xb, yb, block_wet, block_nbr, shape, periodic, fold, halo, explicit):
    """What mask_table() returns: masked ((n, 2) int32: a, b of the masked blocks in ascending (b, a)), block_wet and block_nbr ((py,
    px) int32), xbegin and ybegin, and the record of the layout formed from them on the host."""
    ny, nx = shape
    sx = np.diff(np.append(xb, nx))
    sy = np.diff(np.append(yb, ny))
    m = block_nbr == 0
    b, a = np.nonzero(m)   # row-major: ascending (b, a)
    status = 0
    if fold and np.any(xb + (np.append(xb, nx)[1:] - 1)[::-1] != nx - 1):
        status |= L.LAYOUT_FOLD_ASYMMETRIC
    rec = dict(px=int(px), py=int(py), blocks=int(px * py), masked=int(m.sum()), pes=int(px * py - m.sum()),
               max_block_cells=int(sx.max() * sy.max()), max_block_edge=int(sx.max() + sy.max()), min_block_size=int(min(sx.min(), sy.min())),
               max_wet=int(block_wet.max()), masked_cells=int((np.outer(sy, sx) * m).sum()), wet_total=int(block_wet.sum()), status=status)
    return {"px": int(px), "py": int(py), "masked": np.stack([a, b], axis=1).astype(np.int32), "block_wet": block_wet, "block_nbr": block_nbr,
            "xbegin": np.asarray(xb, np.int32), "ybegin": np.asarray(yb, np.int32), "max_sizes": [int(sx.max()), int(sy.max())],
            "record": rec, "shape": [int(ny), int(nx)], "periodic": bool(periodic), "fold": bool(fold), "halo": int(halo),
            "explicit": bool(explicit)}


def _check_layout(px, py, shape):
    px, py = int(px), int(py)
    if not (1 <= px <= min(shape[1], L.LAYOUT_MAX_DIV) and 1 <= py <= min(shape[0], L.LAYOUT_MAX_DIV)):
        raise ValueError("mask table: the layout %d x %d does not fit %d x %d cells (at most %d blocks either way)"
                         % (px, py, shape[1], shape[0], L.LAYOUT_MAX_DIV))
    return px, py


# ---- host arrays -----------------------------------------------------------------------------------------------
def layouts(wet, candidates=None, max_blocks=None, periodic=False, fold=False, halo=0, min_block=2):
    """The records of the candidate layouts of the wet set ``wet`` ((ny, nx), 0: land) on one GPU through the host-pointer entry
    ogg_layouts.  candidates: (px, py) pairs, or None for sweep_candidates(ny, nx, max_blocks, min_block).  A dict: records (a RECORD
    array: px, py and the fields of ogg_layout_record), shape, periodic, fold, halo, max_blocks, min_block."""
    wet = np.asarray(wet)
    m = F.wet_mask(wet, wet.shape, "layouts")
    cand = _candidates_for(m.shape, candidates, max_blocks, min_block)
    p = params(m.shape[0], m.shape[1], periodic, fold, halo, cand)
    rec = np.zeros(cand.shape[0], L.LAYOUT_RECORD)
    L.call("ogg_layouts", ctypes.byref(p), m.ctypes.data, cand.ctypes.data if cand.size else None, cand.shape[0],
           rec.ctypes.data if cand.size else None, 0, 0, None, None, None, None)
    return _sweep_result(_joined(cand, rec), m.shape, periodic, fold, halo, max_blocks, min_block)


def mask_table(wet, px, py, periodic=False, fold=False, halo=0, xextent=None, yextent=None):
    """The mask table of the layout (px, py) of the wet set ``wet``: see _table_result.  xextent, yextent: None for the rule's
    extents, else the px (py) block sizes of the model's own decomposition, as FMS's xextent and yextent."""
    wet = np.asarray(wet)
    m = F.wet_mask(wet, wet.shape, "mask table")
    px, py = _check_layout(px, py, m.shape)
    p = params(m.shape[0], m.shape[1], periodic, fold, halo)
    xb, yb = _begins(xextent, m.shape[1], px, "xextent"), _begins(yextent, m.shape[0], py, "yextent")
    bw, bn = np.empty((py, px), np.int32), np.empty((py, px), np.int32)
    L.call("ogg_layouts", ctypes.byref(p), m.ctypes.data, None, 0, None, px, py, None if xb is None else xb.ctypes.data,
           None if yb is None else yb.ctypes.data, bw.ctypes.data, bn.ctypes.data)
    return _table_result(px, py, extent(m.shape[1], px)[0] if xb is None else xb, extent(m.shape[0], py)[0] if yb is None else yb, bw, bn,
                         m.shape, periodic, fold, halo, xb is not None or yb is not None)


# ---- device arrays ---------------------------------------------------------------------------------------------
class DeviceTable(object):
    """The summed-area table of a wet set in device memory (ogg_layout_table_dev on the current stream), for any number of sweeps and
    block reports.  wet: a (ny, nx) uint8 device tensor or a host array."""

    def __init__(self, wet, periodic=False, fold=False, halo=0, device=None):
        import torch
        if not hasattr(wet, "data_ptr"):
            w = np.asarray(wet)
            wet = torch.from_numpy(F.wet_mask(w, w.shape, "layouts")).to(device or "cuda")
        if wet.dim() != 2:
            raise ValueError("layouts: the wet mask is %s, not (ny, nx)" % (tuple(wet.shape),))
        self.torch, self.dev = torch, wet.device
        self.wet = (wet != 0).to(torch.uint8).contiguous()
        self.shape = (int(wet.shape[0]), int(wet.shape[1]))
        self.periodic, self.fold, self.halo = bool(periodic), bool(fold), int(halo)
        self.p = params(self.shape[0], self.shape[1], periodic, fold, halo)
        self.wsb = int(L.load().ogg_layout_workspace_bytes(ctypes.byref(self.p)))
        self.ws = torch.empty(self.wsb, dtype=torch.uint8, device=self.dev)
        L.call("ogg_layout_table_dev", ctypes.byref(self.p), self.wet.data_ptr(), self.ws.data_ptr(), self.wsb, self._stream())

    def _stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def sweep(self, cand):
        """the ogg_layout_record array of the candidates (ogg_layout_candidate records, host)"""
        torch = self.torch
        params(self.shape[0], self.shape[1], self.periodic, self.fold, self.halo, cand)
        if cand.shape[0] == 0:
            return np.zeros(0, L.LAYOUT_RECORD)
        dc = torch.from_numpy(cand.view(np.int32).reshape(-1, 2)).to(self.dev)
        dr = torch.empty((cand.shape[0], len(L.LAYOUT_RECORD_FIELDS)), dtype=torch.int32, device=self.dev)
        L.call("ogg_layout_sweep_dev", ctypes.byref(self.p), dc.data_ptr(), cand.shape[0], self.ws.data_ptr(), self.wsb, dr.data_ptr(),
               self._stream())
        return np.ascontiguousarray(dr.cpu().numpy()).view(L.LAYOUT_RECORD).reshape(-1)

    def blocks(self, px, py, xb=None, yb=None):
        """(block_wet, block_nbr) of one layout as (py, px) int32 host arrays; xb, yb: None or explicit begins (int32, host)"""
        torch = self.torch
        bw, bn = (torch.empty((py, px), dtype=torch.int32, device=self.dev) for _ in range(2))
        L.call("ogg_layout_blocks_dev", ctypes.byref(self.p), px, py, None if xb is None else xb.ctypes.data,
               None if yb is None else yb.ctypes.data, self.ws.data_ptr(), self.wsb, bw.data_ptr(), bn.data_ptr(), self._stream())
        return bw.cpu().numpy(), bn.cpu().numpy()


def layouts_dev(wet, candidates=None, max_blocks=None, periodic=False, fold=False, halo=0, min_block=2, table=None):
    """layouts() with the wet set as a device tensor (or a DeviceTable built before as ``table``): the same dict"""
    t = table if table is not None else DeviceTable(wet, periodic, fold, halo)
    cand = _candidates_for(t.shape, candidates, max_blocks, min_block)
    return _sweep_result(_joined(cand, t.sweep(cand)), t.shape, t.periodic, t.fold, t.halo, max_blocks, min_block)


def mask_table_dev(wet, px, py, periodic=False, fold=False, halo=0, xextent=None, yextent=None, table=None):
    """mask_table() with the wet set as a device tensor (or a DeviceTable built before as ``table``): the same dict"""
    t = table if table is not None else DeviceTable(wet, periodic, fold, halo)
    px, py = _check_layout(px, py, t.shape)
    xb, yb = _begins(xextent, t.shape[1], px, "xextent"), _begins(yextent, t.shape[0], py, "yextent")
    bw, bn = t.blocks(px, py, xb, yb)
    return _table_result(px, py, extent(t.shape[1], px)[0] if xb is None else xb, extent(t.shape[0], py)[0] if yb is None else yb, bw, bn,
                         t.shape, t.periodic, t.fold, t.halo, xb is not None or yb is not None)


# ---- ranking -----------------------------------------------------------------------------------------------------
def _key(r):
    return (int(r["max_block_cells"]), int(r["max_block_edge"]), int(r["blocks"]), int(r["px"]))


def record_dict(r):
    return {f: int(r[f]) for f in RECORD.names}


def best_layouts(records, target_pes):
    """Among the records (a RECORD array, or a layouts() result) with status == 0: ``best``, the one with pes == target_pes and the
    smallest key (max_block_cells, max_block_edge, blocks, px), or None; ``by_pes``, the best record of every pes <= target_pes in
    descending pes (the near misses).  Records as dicts of Python ints."""
    if isinstance(records, dict):
        records = records["records"]
    target_pes = int(target_pes)
    if target_pes < 1:
        raise ValueError("layouts: the target must be >= 1 process, not %d" % target_pes)
    by = {}
    ok = records[(records["status"] == 0) & (records["pes"] <= target_pes)]
    for r in ok:
        pes = int(r["pes"])
        if pes not in by or _key(r) < _key(by[pes]):
            by[pes] = r
    best = by.get(target_pes)
    return {"target_pes": target_pes, "best": None if best is None else record_dict(best),
            "by_pes": [record_dict(by[k]) for k in sorted(by, reverse=True)]}


# ---- files -----------------------------------------------------------------------------------------------------
def default_name(count, px, py):
    return "mask_table.%d.%dx%d" % (count, px, py)


def table_text(px, py, masked):
    """FMS's text: the count of masked blocks, ``px,py``, then one 1-based ``i,j`` line per masked block"""
    return "%d\n%d,%d\n" % (len(masked), px, py) + "".join("%d,%d\n" % (int(a) + 1, int(b) + 1) for a, b in masked)


def write_mask_table(path, table, py=None, masked=None):
    """Write a mask table: ``table`` a mask_table() result, or px with py and masked (0-based (a, b) pairs in ascending (b, a)).
    ``path``: the file, or a directory, in which the file gets its default name mask_table.<count>.<px>x<py>.  The path written."""
    if isinstance(table, dict):
        px, py, masked = table["px"], table["py"], table["masked"]
    else:
        px = int(table)
    path = str(path)
    if os.path.isdir(path):
        path = os.path.join(path, default_name(len(masked), px, py))
    with open(path, "w") as fh:
        fh.write(table_text(px, py, masked))
    return path


def read_mask_table(path):
    """(px, py, masked) of a mask table file: masked an (n, 2) int32 array of 0-based (a, b)"""
    lines = [ln.strip() for ln in open(str(path)).read().splitlines() if ln.strip()]
    try:
        n = int(lines[0])
        px, py = (int(v) for v in lines[1].split(","))
        masked = np.array([[int(v) - 1 for v in ln.split(",")] for ln in lines[2:]], dtype=np.int32).reshape(-1, 2)
    except (IndexError, ValueError):
        raise ValueError("%s: not a mask table (the count, then px,py, then one i,j per line)" % path)
    if masked.shape[0] != n or (n and (masked.min() < 0 or masked[:, 0].max() >= px or masked[:, 1].max() >= py)):
        raise ValueError("%s: %d blocks listed for a count of %d in a %d x %d layout" % (path, masked.shape[0], n, px, py))
    return px, py, masked


def summary_lines(table):
    """LAYOUT and MASKTABLE as MOM6's input takes them, the processes saved, the largest block and the busiest block"""
    r = table["record"]
    out = ["   layout: LAYOUT = %d,%d" % (table["px"], table["py"]),
           "   layout: MASKTABLE = %s" % default_name(r["masked"], table["px"], table["py"]),
           "   layout: %d of %d blocks hold no ocean%s: %d processes instead of %d (%.1f %% saved), %d of %d cells masked"
           % (r["masked"], r["blocks"], " within a halo of %d" % table["halo"] if table["halo"] else "", r["pes"], r["blocks"],
              100.0 * r["masked"] / r["blocks"], r["masked_cells"], table["shape"][0] * table["shape"][1]),
           "   layout: the largest block is %d x %d cells%s; the busiest block holds %d wet cells (%.1f %% of the largest block)"
           % (table["max_sizes"][0], table["max_sizes"][1], " (explicit extents)" if table["explicit"] else "", r["max_wet"],
              100.0 * r["max_wet"] / r["max_block_cells"])]
    if r["status"] & L.LAYOUT_FOLD_ASYMMETRIC:
        out.append("   layout: WARNING: the x extents are not mirror images across the fold; FMS refuses such a decomposition of a tripolar grid")
    return out


def sweep_lines(res, ranking):
    rec = res["records"]
    out = ["   layout: %d layouts of at most %d blocks (blocks of at least %d cells a side, halo %d) on %d x %d cells: %d usable"
           % (rec.shape[0], res["max_blocks"], res["min_block"], res["halo"], res["shape"][1], res["shape"][0], int((rec["status"] == 0).sum()))]
    if ranking is not None:
        b = ranking["best"]
        if b is None:
            near = ranking["by_pes"][0] if ranking["by_pes"] else None
            out.append("   layout: no layout runs on exactly %d processes%s" % (ranking["target_pes"], "" if near is None else
                       "; the nearest below is %d,%d on %d" % (near["px"], near["py"], near["pes"])))
        else:
            out.append("   layout: for %d processes the smallest blocks come with %d,%d: %d blocks, %d masked, %d cells in the largest block"
                       % (ranking["target_pes"], b["px"], b["py"], b["blocks"], b["masked"], b["max_block_cells"]))
    return out


# ---- the flags of main() and of the file command ------------------------------------------------------------------
def wanted(a):
    """whether the flag record ``a`` (attributes named as FLAG_DEFAULTS) asks for any layout work"""
    return bool(a.mask_table_layout) or a.layout_sweep is not None


def validate_flags(a, topog_source):
    """Every refusal of the layout flags, before any device work (ValueError)"""
    if a.layout_halo is None or int(a.layout_halo) < 0:
        raise ValueError("--layout_halo must be >= 0, not %r" % (a.layout_halo,))
    if a.layout_min_block is None or int(a.layout_min_block) < 1:
        raise ValueError("--layout_min_block must be >= 1, not %r" % (a.layout_min_block,))
    if not wanted(a):
        if (a.mask_table_dir or a.layout_target_pes is not None or a.layout_report or a.layout_xextent or a.layout_yextent
                or int(a.layout_halo) != 0 or int(a.layout_min_block) != 2):
            raise ValueError("--mask_table_dir, --layout_target_pes, --layout_report, --layout_halo, --layout_min_block, --layout_xextent and "
                             "--layout_yextent need --mask_table_layout or --layout_sweep")
        return
    if topog_source is None:
        raise ValueError("--mask_table_layout and --layout_sweep need --topog_source: the masked blocks are those of the topography's wet cells")
    for pair in a.mask_table_layout or ():
        if len(pair) != 2 or int(pair[0]) < 1 or int(pair[1]) < 1:
            raise ValueError("--mask_table_layout takes PX PY, both >= 1, not %r" % (tuple(pair),))
    if a.layout_sweep is not None and int(a.layout_sweep) < 1:
        raise ValueError("--layout_sweep must be >= 1 block, not %r" % (a.layout_sweep,))
    if a.layout_target_pes is not None:
        if a.layout_sweep is None:
            raise ValueError("--layout_target_pes needs --layout_sweep: the target is met by one of the sweep's layouts")
        if int(a.layout_target_pes) < 1:
            raise ValueError("--layout_target_pes must be >= 1, not %r" % (a.layout_target_pes,))
    if (a.layout_xextent or a.layout_yextent) and len(a.mask_table_layout or ()) != 1:
        raise ValueError("--layout_xextent and --layout_yextent need exactly one --mask_table_layout: they are the extents of that layout")
    for name, v in (("--layout_xextent", a.layout_xextent), ("--layout_yextent", a.layout_yextent)):
        if v:
            parse_extent(name, v)


def parse_extent(name, text):
    """the block sizes of a comma list"""
    if not isinstance(text, str):
        return [int(v) for v in text]
    try:
        return [int(v) for v in text.split(",")]
    except ValueError:
        raise ValueError("%s takes a comma list of block sizes, not %r" % (name, text))


def run_flags(a, sweep, table):
    """What main() and the file command do with the layout flags ``a``: the explicit layouts' tables, the sweep, its ranking and the
    winner's table, each printed and written as it is done, and the report.  sweep(**kw) -> a layouts() result, table(px, py, **kw) ->
    a mask_table() result; either returns None on a rank that holds no result, and nothing is written there."""
    halo, outdir = int(a.layout_halo), str(a.mask_table_dir or ".")
    report = {"tables": [], "sweep": None}
    tables = []
    for k, (px, py) in enumerate(a.mask_table_layout or ()):
        kw = {}
        if a.layout_xextent:
            kw["xextent"] = parse_extent("--layout_xextent", a.layout_xextent)
        if a.layout_yextent:
            kw["yextent"] = parse_extent("--layout_yextent", a.layout_yextent)
        t = table(int(px), int(py), halo=halo, **kw)
        if t is None:
            return None
        tables.append(t)
    if a.layout_sweep is not None:
        res = sweep(max_blocks=int(a.layout_sweep), halo=halo, min_block=int(a.layout_min_block))
        if res is None:
            return None
        ranking = None if a.layout_target_pes is None else best_layouts(res, a.layout_target_pes)
        for line in sweep_lines(res, ranking):
            print(line)
        report["sweep"] = {k: res[k] for k in ("shape", "periodic", "fold", "halo", "max_blocks", "min_block")}
        report["sweep"]["candidates"] = int(res["records"].shape[0])
        if ranking is not None:
            report["sweep"].update(ranking)
            if ranking["best"] is not None and not a.mask_table_layout:
                tables.append(table(ranking["best"]["px"], ranking["best"]["py"], halo=halo))
    if tables:
        os.makedirs(outdir, exist_ok=True)
    for t in tables:
        for line in summary_lines(t):
            print(line)
        path = write_mask_table(outdir, t)
        print("   layout: wrote %s" % path)
        report["tables"].append(dict(t["record"], file=os.path.basename(path), explicit=t["explicit"], xbegin=t["xbegin"].tolist(),
                                     ybegin=t["ybegin"].tolist(), masked=t["masked"].tolist()))
    if a.layout_report:
        with open(str(a.layout_report), "w") as fh:
            json.dump(report, fh, indent=1)
    return report


def add_flags(parser):
    """the layout flags of main()'s parser and of the file command's"""
    parser.add_argument("--mask_table_layout", type=int, nargs=2, action="append", required=False, default=None, metavar=("PX", "PY"),
                        help="write the FMS mask table of the layout PX,PY (repeatable): the blocks without a wet cell of the "
                             "--topog_source topography (the --ocean_mask_file mask when given)")
    parser.add_argument("--mask_table_dir", type=str, required=False, default=None,
                        help="the directory of the mask tables, each named mask_table.<count>.<px>x<py> (default: the working directory)")
    parser.add_argument("--layout_sweep", type=int, required=False, default=None, metavar="MAX_BLOCKS",
                        help="form the record of every layout of at most MAX_BLOCKS blocks")
    parser.add_argument("--layout_target_pes", type=int, required=False, default=None, metavar="T",
                        help="among the sweep's layouts that run on exactly T processes after masking, name the one with the smallest "
                             "blocks and, without --mask_table_layout, write its table")
    parser.add_argument("--layout_report", type=str, required=False, default=None, help="write the sweep's ranking and the tables as JSON to this file")
    parser.add_argument("--layout_halo", type=int, required=False, default=0, metavar="H",
                        help="a block is masked only when no wet cell lies within H cells of it (default 0)")
    parser.add_argument("--layout_min_block", type=int, required=False, default=2, metavar="N",
                        help="the sweep leaves out layouts with a block of fewer than N cells a side (default 2)")
    parser.add_argument("--layout_xextent", type=str, required=False, default=None,
                        help="the block sizes along x of the one --mask_table_layout, a comma list, instead of the rule's")
    parser.add_argument("--layout_yextent", type=str, required=False, default=None, help="the same along y")


def main(argv=None):
    from . import netcdf3
    from . import ocean_mask as M
    from . import remap as R
    p = argparse.ArgumentParser(prog="python -m ocean_model_grid_generator_amd.layout",
                                description="processor layouts and FMS mask tables of the wet set of a topography or an ocean mask")
    g = p.add_mutually_exclusive_group(required=True)
    g.add_argument("--topog", default=None, help="topog.nc: cells with depth > 0 are wet")
    g.add_argument("--mask", default=None, help="ocean_mask.nc: cells with mask != 0 are wet")
    p.add_argument("--grid", default=None, help="ocean_hgrid.nc: the periodic seam and the fold are read from its corner points")
    p.add_argument("--periodic", action="store_true", help="without --grid: the grid is periodic in x")
    p.add_argument("--fold", action="store_true", help="without --grid: the top row is folded (a tripolar grid)")
    add_flags(p)
    a = p.parse_args(argv)
    if a.grid and (a.periodic or a.fold):
        raise ValueError("--periodic and --fold state the topology without --grid; with --grid it is read from the corner points")
    validate_flags(a, a.topog or a.mask)
    if not wanted(a):
        raise ValueError("nothing to do: give --mask_table_layout or --layout_sweep")
    wet = R.mask_from_file(a.topog or a.mask)
    periodic, fold = a.periodic, a.fold
    if a.grid:
        xy = netcdf3.read_doubles(a.grid, names=("x", "y"))
        if xy["x"].shape != (2 * wet.shape[0] + 1, 2 * wet.shape[1] + 1):
            raise ValueError("%s holds %s points, the wet set %s cells" % (a.grid, xy["x"].shape, wet.shape))
        periodic, fold = M.detect_topology(xy["x"], xy["y"], 2)
    return run_flags(a, lambda **kw: layouts(wet, periodic=periodic, fold=fold, **kw),
                     lambda px, py, **kw: mask_table(wet, px, py, periodic=periodic, fold=fold, **kw))


if __name__ == "__main__":
    main()
    sys.exit(0)
