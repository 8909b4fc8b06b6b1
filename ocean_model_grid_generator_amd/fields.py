"""Fields on files: what the analyses that take a field from a NetCDF file and write their results to one (remap.py, runoff.py,
latlon_regrid.py, bilinear.py) share.  A Field is an array of records of one 2-D grid with its missing values and what a writer
needs to carry its leading dimensions over; the reader is one NetCDF classic / 64-bit-offset variable reader; the writers share the
merge of the leading dimensions of several results; the command lines share their loop over --var and their JSON summary.
"""
import json

import numpy as np

from . import _lib as L
from . import netcdf3

CDF2_VAR_LIMIT = (1 << 32) - 4      # bytes of one fixed-size variable (or one record of a record variable) of a 64-bit-offset file
DTYPES = {np.dtype(np.float32): L.REMAP_FLOAT32, np.dtype(np.float64): L.REMAP_FLOAT64}


class Field(object):
    """A field of records on a 2-D grid: data (..., rows, columns), float32 or float64; the values that mark missing (``fill``, at most
    two, in the data's type; NaN is always missing); the leading dimensions [(name, length)] and their coordinate variables [(name,
    nc type, attributes, values)] for the writer; ``note`` says how it was read; ``record_dim`` the unlimited dimension of the file it
    came from (None: none)."""
    _who = "regrid field"   # the words in front of a refusal

    def __init__(self, data, fill=(), name="field", lead_dims=None, coords=(), atts=(), note="", record_dim=None):
        data = np.asarray(data)
        if data.ndim < 2 or data.dtype.newbyteorder("=") not in DTYPES:
            raise ValueError("%s: a float32 or float64 array of two or more dimensions is needed, not %s %s" % (self._who, data.dtype, data.shape))
        self.data = np.ascontiguousarray(data, dtype=data.dtype.newbyteorder("="))
        self.fill = tuple(self.data.dtype.type(f) for f in fill)
        if len(self.fill) > L.REMAP_MAX_FILLS:
            raise ValueError("%s: at most %d fill values" % (self._who, L.REMAP_MAX_FILLS))
        self.name = name
        lead = self.data.shape[:-2]
        self.lead_dims = list(lead_dims) if lead_dims is not None else [("record%d" % k, n) for k, n in enumerate(lead)]
        self.coords, self.atts, self.note, self.record_dim = list(coords), list(atts), note, record_dim

    @property
    def nrec(self):
        return int(np.prod(self.data.shape[:-2], dtype=np.int64))

    @property
    def records(self):
        """the data as (nrec, rows, columns)"""
        return self.data.reshape((self.nrec,) + self.data.shape[-2:])


def cell_mask(mask, shape, who):
    """None, or ``mask`` as one byte per model cell (0: dry); ``who``: the words in front of the refusal of another shape"""
    if mask is None:
        return None
    m = np.ascontiguousarray(np.asarray(mask) != 0, dtype=np.uint8)
    if m.shape != shape:
        raise ValueError("%s is %s, the model cells %s" % (who, m.shape, shape))
    return m


def wet_mask(wet, shape, who):
    """the wet mask an analysis needs, as cell_mask gives it; ``who``: the analysis, in front of the refusal"""
    if wet is None:
        raise ValueError("%s: a wet mask is needed (depth > 0 of a topography or mask != 0 of an ocean mask)" % who)
    return cell_mask(wet, shape, "%s: the wet mask" % who)


def resolve_topology(periodic, fold, detect):
    """(periodic, fold) as booleans; what the caller left None comes from detect()"""
    if periodic is None or fold is None:
        p, f = detect()
        periodic, fold = (p if periodic is None else periodic), (f if fold is None else fold)
    return bool(periodic), bool(fold)


# ---- reading ---------------------------------------------------------------------------------------------------
def _num(atts, key):
    v = atts.get(key)
    return None if v is None or isinstance(v, str) else float(np.asarray(v).reshape(-1)[0])


NCCOPY = "convert it with `nccopy -k 64-bit-offset IN OUT`"


def uniform_axis(path, name, c):
    """(values, step) of a coordinate variable that is uniform within 1e-9 of its step"""
    c = np.asarray(c, dtype=np.float64).reshape(-1)
    if c.size < 2:
        raise ValueError("%s: coordinate %s has %d values; two or more are needed" % (path, name, c.size))
    step = (c[-1] - c[0]) / (c.size - 1)
    if step == 0 or np.max(np.abs(np.diff(c) - step)) > 1e-9 * abs(step):
        raise ValueError("%s: coordinate %s is not uniform within 1e-9 of its step %r" % (path, name, step))
    return c, step


def axis_edges(c0, step):
    """(first edge, note): coordinates at half-steps of the lattice k * step are cell centres, any others are taken as edges."""
    r = c0 / abs(step) - 0.5
    if abs(r - round(r)) <= 1e-6:
        return c0 - 0.5 * abs(step), "centres"
    return c0, "edges"


_LAT_NAMES, _LON_NAMES = ("lat", "latitude", "y", "nlat"), ("lon", "longitude", "x", "nlon")


def lat_lon_dims(path, h, v):
    """(latitude dimension, longitude dimension) of a 2-D variable, from its coordinate variables' units (degrees_north /
    degrees_east, as CF has them) or, without units, their names; a file where neither decides is refused."""
    kinds = []
    for d in v.dims:
        cv = h.vars.get(d)
        units = cv.atts.get("units", "") if cv is not None else ""
        units = units.strip().lower() if isinstance(units, str) else ""
        if units in ("degrees_north", "degree_north", "degrees_n", "degree_n"):
            kinds.append("lat")
        elif units in ("degrees_east", "degree_east", "degrees_e", "degree_e"):
            kinds.append("lon")
        elif d.lower() in _LAT_NAMES:
            kinds.append("lat")
        elif d.lower() in _LON_NAMES:
            kinds.append("lon")
        else:
            kinds.append(None)
    if sorted(k for k in kinds if k) != ["lat", "lon"]:
        raise ValueError("%s: cannot tell the latitude and longitude dimensions of %s%s: give the coordinate variables units "
                         "degrees_north / degrees_east" % (path, v.name, tuple(v.dims)))
    return (v.dims[0], v.dims[1]) if kinds[0] == "lat" else (v.dims[1], v.dims[0])


def open_variable(path, var, what, records=True):
    """The header of a NetCDF classic (CDF-1) or 64-bit-offset (CDF-2) file and its byte / short / float / double variable ``var`` of
    two or more dimensions.  CDF-5 and NetCDF-4 / HDF5 files are refused (``what``: "sources", "fields" in that refusal), and so is
    a record (unlimited) variable unless ``records``."""
    try:
        h = netcdf3.read_header(path)
    except ValueError as e:
        if "CDF-5" in str(e) or "HDF5" in str(e):
            raise ValueError("%s: only NetCDF classic / 64-bit-offset %s are read; %s" % (str(e).split(";")[0], what, NCCOPY))
        raise
    if var not in h.vars:
        raise KeyError("%s: no variable %r (variables: %s); choose one with --var" % (path, var, ", ".join(sorted(h.vars))))
    v = h.vars[var]
    if v.nc_type not in (netcdf3.NC_BYTE, netcdf3.NC_SHORT, netcdf3.NC_FLOAT, netcdf3.NC_DOUBLE) or len(v.shape) < 2:
        raise ValueError("%s: %s must be a byte, short, float or double variable of two or more dimensions (type %d, shape %s)"
                         % (path, var, v.nc_type, v.shape))
    if v.is_record and not records:
        raise ValueError("%s: %s is a record (unlimited) variable; only fixed-size variables are read" % (path, var))
    return h, v


def read_values(path, h, v, records=True, keep=("units", "long_name")):
    """What a Field holds of the variable v of open_variable(): (data, fill, lead_dims, coords, atts).  A byte or short variable is
    unpacked to float64 as raw * scale_factor + add_offset, with missing values (_FillValue, missing_value, tested on the raw values)
    as NaN; float and double keep their type and their fill values.  Every dimension ahead of the last two is a leading dimension;
    its 1-D numeric coordinate variable is read too (a record one only with ``records``).  ``keep``: the text attributes kept."""
    def raw_bytes(name, u):
        return (netcdf3.read_record_var_bytes if u.is_record else netcdf3.read_var_bytes)(path, h, name, dtype=u.nc_type)
    data = np.frombuffer(raw_bytes(v.name, v), dtype=netcdf3.NUMPY_DTYPE[v.nc_type]).reshape(v.shape)
    data = data.astype(data.dtype.newbyteorder("="))
    fills = []
    for k in ("_FillValue", "missing_value"):
        fv = _num(v.atts, k)
        if fv is not None and fv not in fills:
            fills.append(fv)
    if v.nc_type in (netcdf3.NC_BYTE, netcdf3.NC_SHORT):
        scale, offset = _num(v.atts, "scale_factor"), _num(v.atts, "add_offset")
        miss = np.zeros(data.shape, dtype=bool)
        for fv in fills:
            miss |= data == data.dtype.type(fv)
        out = data.astype(np.float64) * (1.0 if scale is None else scale) + (0.0 if offset is None else offset)
        out[miss] = np.nan
        data, fills = out, []
    lead = [(d, n) for d, n in zip(v.dims[:-2], v.shape[:-2])]
    coords = []
    for d, _ in lead:
        cv = h.vars.get(d)
        if cv is not None and len(cv.shape) == 1 and (records or not cv.is_record) and cv.nc_type != netcdf3.NC_CHAR:
            vals = np.frombuffer(raw_bytes(d, cv), dtype=netcdf3.NUMPY_DTYPE[cv.nc_type])
            atts = [(k, a if isinstance(a, str) else np.asarray(a).reshape(-1)[0].item()) for k, a in cv.atts.items()
                    if isinstance(a, str) or np.asarray(a).size == 1]
            coords.append((d, cv.nc_type, atts, vals))
    return data, fills, lead, coords, [(k, a) for k, a in v.atts.items() if k in keep and isinstance(a, str)]


# ---- writing ---------------------------------------------------------------------------------------------------
def writer_dims(who, entries, advice="", record_dims=False):
    """The leading dimensions of a file that holds several results: ``entries`` [(Field, [(variable name, values), ...])].  A
    dimension with two lengths is refused, and so is a variable (one record of it, under a record dimension) over CDF2_VAR_LIMIT
    (``advice`` ends that refusal).  With ``record_dims`` the fields' record dimension stays the file's: there is one at most, first in
    every variable that has it and first of the dimensions.  (dims, the fields' coordinate variables of them, record dimension or None)."""
    dims, coords, record_dim = [], [], None
    for fld, variables in entries:
        rd = fld.record_dim if record_dims else None
        if rd is not None:
            if record_dim not in (None, rd):
                raise ValueError("%s: two record dimensions, %s and %s" % (who, record_dim, rd))
            record_dim = rd
        for d, n in fld.lead_dims:
            if d in dict(dims):
                if dict(dims)[d] != n:
                    raise ValueError("%s: dimension %s has length %d in one variable and %d in another" % (who, d, dict(dims)[d], n))
                continue
            dims.append((d, n))
            coords += [c for c in fld.coords if c[0] == d]
        for name, values in variables:
            nbytes = int(np.prod(values.shape[1 if rd else 0:], dtype=np.int64)) * 8
            if nbytes > CDF2_VAR_LIMIT:
                raise ValueError("%s: %s takes %d bytes, more than one variable of a NetCDF 64-bit-offset file can hold (%d)%s"
                                 % (who, name, nbytes, CDF2_VAR_LIMIT, advice))
    for fld, _ in entries:
        if record_dim is not None and record_dim in dict(fld.lead_dims) and fld.lead_dims[0][0] != record_dim:
            raise ValueError("%s: %s has the record dimension %s but not first" % (who, fld.name, record_dim))
    if record_dim is not None:   # the record dimension first, as the format wants it
        dims.sort(key=lambda d: d[0] != record_dim)
    return dims, coords, record_dim


# ---- command lines ---------------------------------------------------------------------------------------------
def dump_summaries(path, out):
    """the summaries of [(field(s), result)] as JSON, when a path is given"""
    if path:
        with open(path, "w") as fh:
            json.dump([r["summary"] for _, r in out], fh, indent=1)


def run_variables(names, read, compute, summary_lines, write, output, json_path):
    """The tail of a main(): every variable read (its note printed) and computed (its summary lines printed), the results written to
    ``output`` and their summaries to ``json_path``.  [(field, result)]."""
    out = []
    for var in names:
        fld = read(var)
        print(fld.note)
        res = compute(fld)
        for line in summary_lines(res):
            print(line)
        out.append((fld, res))
    write(output, out)
    dump_summaries(json_path, out)
    return out
