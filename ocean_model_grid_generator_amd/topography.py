"""Topography by refined sampling: the cell mean, spread, extremes and wet fraction of a bathymetry raster on a supergrid, the
``topog.nc`` MOM6 reads (include/ogg_hip.h, "Topography by refined sampling", gives the definition).  The reference has no such step.

Every sample is taken on the device by libogg_hip.so (ogg_topog_band_dev / ogg_topog): one integer record per output cell (counts,
sum q, sum q^2, min, max of the quantised source values q), combined here only by integer sums, minima and maxima, so the result is
bit-identical whatever the split of the grid into bands or ranks.  The floating outputs are a fixed function of those integers.
With ``plane`` (--roughness) the records also carry the integer moments of every cell's least-squares plane ("Plane-fit topography"
in the header): the roughness h2 about that plane and its slope, the resolved bottom slope, come from them.

    python -m ocean_model_grid_generator_amd.topography ocean_hgrid.nc SOURCE [SOURCE ...] -o topog.nc [--var elevation] [--refine R]
        [--oversample F] [--quantum Q] [--sea_level L] [--supergrid_cells] [--roughness] [--json summary.json]
        [--source_box LON0 DLON LAT0 DLAT] [--source_proj stere:S,lat_ts=-71,lon0=0] [--faces topog_faces.nc]

SOURCE is a NetCDF classic / 64-bit-offset file (a short, float or double variable on uniform 1-D lon / lat coordinates) or a .npy
array with --source_box (cell edges: lon0 + is * dlon, lat0 + js * dlat, row 0 southmost).

Several SOURCEs (up to four) are layers in order of priority, and a source may be a polar-stereographic raster in metres (a CF
polar_stereographic grid mapping in the file, or --source_proj): "Layered topography" in the header, ogg_topog_layers_band_dev /
ogg_topog_layers on the device.  Every sample takes the first source that has a value for it, the result also tells how many samples
each source gave (n_from, n_from_source in the file), and the plane fit is not made.
"""
import argparse
import ctypes
import json
import sys

import numpy as np

from . import _lib as L
from . import netcdf3
from .fields import NCCOPY as _NCCOPY, axis_edges as _edges, lat_lon_dims as _lat_lon_dims, uniform_axis as _uniform_axis

NO_PLANE = ("the plane fit (--topog_roughness, --roughness) lives in one lat-lon raster's index space: it is not made from a list of "
            "sources or from a projected source")
FILL = 1.0e20                 # _FillValue of the floating outputs (cells without a valid sample)
DEFAULT_QUANTUM = 0.01        # float sources: q = rint(v / quantum)
RE = 6371.0e3                 # the library's Earth radius (kReDefault of csrc/ogg_math.h): the bottom slopes are per metre
_EMPTY = (0, 0, 0, 0, 0, np.iinfo(np.int32).max, np.iinfo(np.int32).min, 0, 0, 0)   # a record with no sample
_EMPTY_PLANE = _EMPTY + (0,) * len(L.TOPOG_MOMENT_FIELDS)
_DTYPES = {np.dtype(np.int16): L.TOPOG_INT16, np.dtype(np.float32): L.TOPOG_FLOAT32, np.dtype(np.float64): L.TOPOG_FLOAT64}


# ---- sources -------------------------------------------------------------------------------------------------
MIN_LAT_GATE = -80.0          # the lowest gate latitude (h * lat) the library takes


class PolarStereo(object):
    """The polar stereographic projection of a raster in metres ("Layered topography" of include/ogg_hip.h): hemisphere "N" / "S" (or
    +1 / -1), the latitude of true scale ``lat_ts`` and the central meridian ``lon0`` in degrees, the ellipsoid by its semi-major axis
    ``a`` and its inverse flattening ``rf`` (0: a sphere) or its eccentricity ``e``; WGS84 unless given.  K is the header's constant."""

    def __init__(self, hemisphere, lat_ts=None, lon0=0.0, a=6378137.0, rf=298.257223563, e=None):
        h = {"N": 1, "S": -1, 1: 1, -1: -1}.get(hemisphere.upper() if isinstance(hemisphere, str) else hemisphere)
        if h is None:
            raise ValueError("polar stereographic: the hemisphere is N or S (+1 or -1), not %r" % (hemisphere,))
        self.h, self.lon0, self.a = h, float(lon0), float(a)
        self.lat_ts = float(90.0 * h if lat_ts is None else lat_ts)
        if e is None:
            f = 0.0 if not rf else 1.0 / float(rf)
            e = np.sqrt(2.0 * f - f * f)
        self.e = float(e)
        if not (self.a > 0 and np.isfinite(self.a) and 0.0 <= self.e < 0.2 and np.isfinite(self.lon0)):
            raise ValueError("polar stereographic: a = %r must be positive and e = %r in [0, 0.2)" % (a, self.e))
        if not 0.0 < h * self.lat_ts <= 90.0:
            raise ValueError("polar stereographic: lat_ts = %g does not lie in the %s hemisphere" % (self.lat_ts, "NS"[h < 0]))
        self.K = float(self._K())

    def _t(self, phi):
        s, c = np.sin(phi), np.cos(phi)
        return c / (1.0 + s) * np.exp(self.e * np.arctanh(self.e * s))

    def _K(self):
        e = self.e
        if self.h * self.lat_ts == 90.0:
            return 2.0 * self.a / np.sqrt((1.0 + e) ** (1.0 + e) * (1.0 - e) ** (1.0 - e))
        phi = self.h * self.lat_ts * (np.pi / 180.0)
        return self.a * (np.cos(phi) / np.sqrt(1.0 - e * e * np.sin(phi) ** 2)) / self._t(phi)

    def pole_latitude(self, X, Y):
        """h * lat in degrees of the points (X, Y) in metres (Snyder's iteration for the inverse, eq. 7-9)"""
        t = np.hypot(np.asarray(X, dtype=np.float64), np.asarray(Y, dtype=np.float64)) / self.K
        phi = np.pi / 2.0 - 2.0 * np.arctan(t)
        for _ in range(8):
            es = self.e * np.sin(phi)
            phi = np.pi / 2.0 - 2.0 * np.arctan(t * ((1.0 - es) / (1.0 + es)) ** (self.e / 2.0))
        return phi * 180.0 / np.pi

    def descriptor(self, lat_gate):
        return L.TopogProjection(h=self.h, lon0=self.lon0, a=self.a, e=self.e, K=self.K, lat_gate=float(lat_gate))

    def __str__(self):
        return "stere:%s,lat_ts=%.10g,lon0=%.10g,a=%.10g,e=%.12g" % ("NS"[self.h < 0], self.lat_ts, self.lon0, self.a, self.e)

    @classmethod
    def parse(cls, text):
        """A PolarStereo from "stere:S,lat_ts=-71,lon0=0[,a=..,rf=..|e=..]" (--source_proj, --topog_proj)"""
        parts = str(text).split(",")
        if not parts[0].startswith("stere:") or parts[0][6:].upper() not in ("N", "S"):
            raise ValueError("projection %r: stere:N or stere:S, then lat_ts=, lon0=, a=, rf= or e= separated by commas" % (text,))
        kw = {}
        for item in parts[1:]:
            k, _, v = item.partition("=")
            if k.strip() not in ("lat_ts", "lon0", "a", "rf", "e"):
                raise ValueError("projection %r: unknown parameter %r (lat_ts, lon0, a, rf, e)" % (text, k))
            kw[k.strip()] = float(v)
        return cls(parts[0][6:], **kw)


class Source(object):
    """A raster on the host: data (Ny x Nx; int16, float32 or float64, row 0 southmost), its cell edges lon0 + is * dlon,
    lat0 + js * dlat, the raw values that mark missing (``fill``), and the quantum of one integer step (int16: 1, or the
    variable's scale_factor; float: DEFAULT_QUANTUM unless given).  ``note`` says how the box was found.
    ``projection`` (a PolarStereo): the raster lies in that plane, and the four box numbers mean X0, dX, Y0, dY in metres (cell edges,
    row 0 the lowest Y).  ``lat_gate``: samples with h * lat below it are not projected; default: 0.01 degrees below the lowest h * lat
    of the raster's four corners (no sample further out can fall inside); below -80 it is refused."""

    def __init__(self, data, lon0, dlon, lat0, dlat, fill=(), quantum=None, note="", projection=None, lat_gate=None, name=None):
        data = np.asarray(data)
        if data.ndim != 2 or data.dtype.newbyteorder("=") not in _DTYPES:
            raise ValueError("topography source: a 2-D int16, float32 or float64 array is needed, not %s %s" % (data.dtype, data.shape))
        self.data = np.ascontiguousarray(data, dtype=data.dtype.newbyteorder("="))
        self.lon0, self.dlon, self.lat0, self.dlat = float(lon0), float(dlon), float(lat0), float(dlat)
        if not (self.dlon > 0 and self.dlat > 0):
            raise ValueError("topography source: dlon and dlat must be positive (%g, %g); rows go south to north" % (dlon, dlat))
        self.fill = tuple(float(self.data.dtype.type(f)) for f in fill)   # a fill value as the raster's type holds it
        if len(self.fill) > 2:
            raise ValueError("topography source: at most two fill values")
        is_int = self.data.dtype == np.int16
        self.quantum = float(quantum if quantum is not None else (1.0 if is_int else DEFAULT_QUANTUM))
        if not (self.quantum > 0 and np.isfinite(self.quantum)):
            raise ValueError("topography source: the quantum must be positive (%r)" % quantum)
        self.note = note
        self.name = name if name is not None else (note.split(":")[0] if note else "array")
        self.projection, self.lat_gate = projection, None
        if projection is not None:
            Ny, Nx = self.data.shape
            if lat_gate is None:
                xs, ys = np.meshgrid([self.lon0, self.lon0 + Nx * self.dlon], [self.lat0, self.lat0 + Ny * self.dlat])
                lat_gate = float(projection.pole_latitude(xs, ys).min()) - 0.01
            self.lat_gate = float(lat_gate)
            if not MIN_LAT_GATE <= self.lat_gate <= 90.0:
                raise ValueError("topography source: the gate latitude %g (h * lat of the raster's furthest corner, or lat_gate=) is "
                                 "outside [%g, 90]: a polar stereographic raster cannot reach that far" % (self.lat_gate, MIN_LAT_GATE))
        elif lat_gate is not None:
            raise ValueError("topography source: lat_gate belongs to a projected source")

    @property
    def shape(self):
        return self.data.shape

    @property
    def periodic(self):
        return self.projection is None and abs(self.data.shape[1] * self.dlon - 360.0) <= 1e-9

    def replace(self, **kw):
        """this source with some of its constructor's arguments changed"""
        args = dict(data=self.data, lon0=self.lon0, dlon=self.dlon, lat0=self.lat0, dlat=self.dlat, fill=self.fill, quantum=self.quantum,
                    note=self.note, projection=self.projection, lat_gate=self.lat_gate, name=self.name)
        args.update(kw)
        return Source(**args)

    def describe(self):
        """the box and the projection in one line (write_topog's ``sources`` attribute)"""
        box = "%.10g %.10g %.10g %.10g" % (self.lon0, self.dlon, self.lat0, self.dlat)
        if self.projection is None:
            return "%s [latlon, box %s]" % (self.name, box)
        return "%s [%s, gate %.10g, box %s]" % (self.name, self.projection, self.lat_gate, box)

    def descriptor(self, sea_level=0.0):
        Ny, Nx = self.data.shape
        d = L.TopogSource(data=self.data.ctypes.data, dtype=_DTYPES[self.data.dtype], n_fill=len(self.fill), Nx=Nx, Ny=Ny, lon0=self.lon0,
                          dlon=self.dlon, lat0=self.lat0, dlat=self.dlat, quantum=self.quantum, wet_below=float(sea_level) / self.quantum)
        for k, f in enumerate(self.fill):
            d.fill[k] = f
        return d


class DeviceSource(object):
    """A Source uploaded once to one GPU: int16 as it is, a float raster quantised there to int32 (ogg_topog_quantize_dev)."""

    def __init__(self, source, device, sea_level=0.0):
        import torch
        self.source, self.device, self.sea_level = source, torch.device(device), float(sea_level)
        raw = torch.from_numpy(source.data).to(self.device)
        d = source.descriptor(sea_level)
        if source.data.dtype == np.int16:
            self.tensor = raw
        else:
            st = torch.cuda.current_stream(self.device).cuda_stream
            q = torch.empty(source.data.shape, dtype=torch.int32, device=self.device)
            bad = torch.zeros(1, dtype=torch.int32, device=self.device)
            d.data = raw.data_ptr()
            L.call("ogg_topog_quantize_dev", ctypes.byref(d), q.data_ptr(), bad.data_ptr(), st)
            if int(bad.item()) != 0:
                raise ValueError("topography source: a value / quantum exceeds 2^21 in magnitude; use a larger --quantum than %g"
                                 % source.quantum)
            del raw
            self.tensor = q
            d.dtype, d.n_fill = L.TOPOG_INT32, 0
        d.data = self.tensor.data_ptr()
        self.desc = d


class SourceList(object):
    """An ordered list of 1 .. 4 Sources, the first with a value for a sample giving it ("Layered topography" of include/ogg_hip.h).
    The list's quantum is the smallest of the sources'; every other quantum must be an integer multiple of it within 1e-9, and that
    multiple is the layer's q_mul (an int16 metre raster under a 0.01 m float raster: q_mul = 100)."""

    def __init__(self, sources):
        self.sources = list(sources)
        if not 1 <= len(self.sources) <= L.TOPOG_MAX_SOURCES:
            raise ValueError("topography: 1 .. %d sources, not %d" % (L.TOPOG_MAX_SOURCES, len(self.sources)))
        self.quantum = min(s.quantum for s in self.sources)
        self.q_mul = []
        for s in self.sources:
            r = s.quantum / self.quantum
            if abs(r - np.rint(r)) > 1e-9 or np.rint(r) > L.TOPOG_MAX_Q:
                raise ValueError("topography: the quantum %g of %s is not an integer multiple of the smallest quantum %g of the list; "
                                 "give the sources quanta that are (--quantum, once per source)" % (s.quantum, s.name, self.quantum))
            self.q_mul.append(int(np.rint(r)))
        self.names = [s.name for s in self.sources]

    def layers(self, sea_level=0.0, descs=None):
        """the ogg_topog_layer array of the list (``descs``: the sources' descriptors when they are not the host ones)"""
        arr = (L.TopogLayer * len(self.sources))()
        for k, s in enumerate(self.sources):
            arr[k].src = s.descriptor(sea_level) if descs is None else descs[k]
            arr[k].src.wet_below = float(sea_level) / self.quantum   # of the list: only layer 0's is read
            arr[k].kind = L.TOPOG_LATLON if s.projection is None else L.TOPOG_POLAR_STEREO
            arr[k].q_mul = self.q_mul[k]
            if s.projection is not None:
                arr[k].proj = s.projection.descriptor(s.lat_gate)
        return arr

    def summary(self):
        return [{"name": s.name, "shape": list(s.shape), "dtype": str(s.data.dtype), "box": [s.lon0, s.dlon, s.lat0, s.dlat],
                 "projection": None if s.projection is None else str(s.projection), "lat_gate": s.lat_gate, "quantum": s.quantum,
                 "q_mul": m} for s, m in zip(self.sources, self.q_mul)]


class DeviceSourceList(object):
    """A SourceList uploaded once to one GPU (every source as a DeviceSource), with the range of q_mul * q checked there"""

    def __init__(self, sources, device, sea_level=0.0):
        import torch
        self.source, self.device, self.sea_level = sources, torch.device(device), float(sea_level)
        self.parts = [DeviceSource(s, device, sea_level) for s in sources.sources]
        self.desc = sources.layers(sea_level, [p.desc for p in self.parts])
        bad = torch.zeros(1, dtype=torch.int32, device=self.device)
        st = torch.cuda.current_stream(self.device).cuda_stream
        for k in range(len(self.parts)):
            L.call("ogg_topog_layer_range_dev", ctypes.byref(self.desc[k]), bad.data_ptr(), st)
            if int(bad.item()) != 0:
                raise ValueError("topography source %s: a value times q_mul = %d exceeds 2^21 in the list's quantum %g; use larger quanta"
                                 % (sources.names[k], sources.q_mul[k], sources.quantum))


def as_sources(source, **kw):
    """What topography() samples: a Source (one lat-lon raster: the single-source entry points, as ever) or a SourceList (a list of
    more than one, or a projected source).  ``source``: a Source, a SourceList, an array with its box, or a list of Sources."""
    if isinstance(source, SourceList):
        return source
    if isinstance(source, (list, tuple)):
        srcs = [as_source(s, **kw) for s in source]
    else:
        srcs = [as_source(source, **kw)]
    if len(srcs) == 1 and srcs[0].projection is None:
        return srcs[0]
    return SourceList(srcs)


def _stereo_mapping(h, v):
    """The PolarStereo of a CF grid mapping of variable ``v`` (grid_mapping_name = polar_stereographic), or None without one"""
    gm = v.atts.get("grid_mapping")
    if not isinstance(gm, str) or gm not in h.vars:
        return None
    at = h.vars[gm].atts
    if at.get("grid_mapping_name") != "polar_stereographic":
        raise ValueError("grid mapping %s: only polar_stereographic is read (%r)" % (gm, at.get("grid_mapping_name")))
    num = lambda k, d=None: float(np.asarray(at[k]).reshape(-1)[0]) if k in at else d   # noqa: E731
    origin = num("latitude_of_projection_origin", None)
    lat_ts = num("standard_parallel", origin)
    if lat_ts is None:
        raise ValueError("grid mapping %s: neither standard_parallel nor latitude_of_projection_origin" % gm)
    hemi = "S" if (origin if origin is not None else lat_ts) < 0 else "N"
    return PolarStereo(hemi, lat_ts, num("straight_vertical_longitude_from_pole", 0.0), num("semi_major_axis", 6378137.0),
                       num("inverse_flattening", 298.257223563))


def _read_source_stereo(path, h, v, var, proj, quantum):
    """read_source_nc for a variable on 1-D x / y coordinates in metres"""
    axes = []
    for dname in v.dims:
        if dname not in h.vars:
            raise ValueError("%s: no coordinate variable for dimension %s of %s" % (path, dname, var))
        cv = h.vars[dname]
        raw = netcdf3.read_var_bytes(path, h, dname, dtype=cv.nc_type)
        axes.append(_uniform_axis(path, dname, np.frombuffer(raw, dtype=netcdf3.NUMPY_DTYPE[cv.nc_type])))
    data = np.frombuffer(netcdf3.read_var_bytes(path, h, var, dtype=v.nc_type), dtype=netcdf3.NUMPY_DTYPE[v.nc_type]).reshape(v.shape)
    data = data.astype(data.dtype.newbyteorder("="))
    first_is_x = v.dims[0].lower().startswith("x") and not v.dims[1].lower().startswith("x")
    if first_is_x:   # stored (x, y): rows are y here
        data, axes = np.ascontiguousarray(data.T), axes[::-1]
    (yc, dy), (xc, dx) = axes
    if dx < 0:
        data, xc, dx = data[:, ::-1], xc[::-1], -dx
    if dy < 0:   # BedMachine's y descends
        data, yc, dy = data[::-1], yc[::-1], -dy
    fill = _fill_values(v)
    if quantum is None and v.nc_type == netcdf3.NC_SHORT and "scale_factor" in v.atts:
        quantum = float(np.asarray(v.atts["scale_factor"]).reshape(-1)[0])
    X0, Y0 = float(xc[0]) - 0.5 * dx, float(yc[0]) - 0.5 * dy   # projected coordinates are cell centres
    note = "%s: %s %s x %s, %s, x and y taken as cell centres: box X0 %.10g dX %.10g Y0 %.10g dY %.10g" % (
        path, var, data.shape[0], data.shape[1], proj, X0, dx, Y0, dy)
    return Source(data, X0, dx, Y0, dy, fill=fill, quantum=quantum, note=note, projection=proj)


def _fill_values(v):
    fill = []
    for k in ("_FillValue", "missing_value"):
        if k in v.atts and not isinstance(v.atts[k], str):
            fv = float(np.asarray(v.atts[k]).reshape(-1)[0])
            if fv not in fill:
                fill.append(fv)
    return fill


def read_source_nc(path, var="elevation", quantum=None, projection=None):
    """A Source from a NetCDF classic (CDF-1) or 64-bit-offset (CDF-2) file: the short / float / double variable ``var`` of
    dimensions (lat, lon) or (lon, lat) (told apart by the coordinates' units or names), its box from the 1-D coordinate variables of those dimensions (uniform within 1e-9 of their step; cell
    centres or edges, as ``note`` says); rows are flipped when latitude decreases.  _FillValue / missing_value mark missing values;
    a short variable's scale_factor is its quantum.  CDF-5 and NetCDF-4 / HDF5 files are refused.
    A variable whose ``grid_mapping`` names a CF polar_stereographic mapping (standard_parallel,
    straight_vertical_longitude_from_pole, semi_major_axis, inverse_flattening), or any variable with ``projection`` (a PolarStereo),
    is read on its 1-D x / y coordinates in metres (cell centres; a descending y is flipped) as a projected Source.  ``projection``
    "latlon" reads the variable as a lat-lon raster whatever grid mapping it names."""
    try:
        h = netcdf3.read_header(path)
    except ValueError as e:
        if "CDF-5" in str(e) or "HDF5" in str(e):
            raise ValueError("%s: only NetCDF classic / 64-bit-offset sources are read; %s" % (str(e).split(";")[0], _NCCOPY))
        raise
    if var not in h.vars:
        raise KeyError("%s: no variable %r (variables: %s); choose one with --var" % (path, var, ", ".join(sorted(h.vars))))
    v = h.vars[var]
    if v.nc_type not in (netcdf3.NC_SHORT, netcdf3.NC_FLOAT, netcdf3.NC_DOUBLE) or len(v.shape) != 2:
        raise ValueError("%s: %s must be a 2-D short, float or double variable (type %d, shape %s)" % (path, var, v.nc_type, v.shape))
    if "add_offset" in v.atts and float(np.asarray(v.atts["add_offset"]).reshape(-1)[0]) != 0.0:
        raise ValueError("%s: %s has a non-zero add_offset, which is not supported" % (path, var))
    projection = None if projection == "latlon" else (projection or _stereo_mapping(h, v))
    if projection is not None:
        return _read_source_stereo(path, h, v, var, projection, quantum)
    lat_name, lon_name = _lat_lon_dims(path, h, v)
    axes = {}
    for dname in (lat_name, lon_name):
        if dname not in h.vars:
            raise ValueError("%s: no coordinate variable for dimension %s of %s" % (path, dname, var))
        cv = h.vars[dname]
        raw = netcdf3.read_var_bytes(path, h, dname, dtype=cv.nc_type)
        axes[dname] = _uniform_axis(path, dname, np.frombuffer(raw, dtype=netcdf3.NUMPY_DTYPE[cv.nc_type]))
    data = np.frombuffer(netcdf3.read_var_bytes(path, h, var, dtype=v.nc_type), dtype=netcdf3.NUMPY_DTYPE[v.nc_type]).reshape(v.shape)
    data = data.astype(data.dtype.newbyteorder("="))
    if v.dims[0] == lon_name:   # stored (lon, lat): rows are latitudes here
        data = np.ascontiguousarray(data.T)
    (lat, dlat), (lon, dlon) = axes[lat_name], axes[lon_name]
    if dlon < 0:
        raise ValueError("%s: longitude %s decreases" % (path, lon_name))
    if dlat < 0:
        data, lat, dlat = data[::-1], lat[::-1], -dlat
    fill = _fill_values(v)
    if quantum is None and v.nc_type == netcdf3.NC_SHORT and "scale_factor" in v.atts:
        quantum = float(np.asarray(v.atts["scale_factor"]).reshape(-1)[0])
    lon0, kind_lon = _edges(lon[0], dlon)
    lat0, kind_lat = _edges(lat[0], dlat)
    note = "%s: %s %s x %s, longitude coordinates taken as cell %s, latitude as cell %s: box lon0 %.10g dlon %.10g lat0 %.10g dlat %.10g" % (
        path, var, data.shape[0], data.shape[1], kind_lon, kind_lat, lon0, dlon, lat0, dlat)
    return Source(data, lon0, dlon, lat0, dlat, fill=fill, quantum=quantum, note=note)


def read_source_npy(path, box, quantum=None, fill=(), projection=None):
    """A Source from a .npy array (Ny x Nx, row 0 southmost) with its box (lon0, dlon, lat0, dlat) of cell edges; with ``projection``
    (a PolarStereo) the box is X0, dX, Y0, dY in metres and row 0 has the lowest Y."""
    if box is None or len(box) != 4:
        raise ValueError("%s: a .npy source needs --source_box LON0 DLON LAT0 DLAT (cell edges)" % path)
    data = np.load(path)
    return Source(data, *box, fill=fill, quantum=quantum, projection=projection,
                  note="%s: %s %s, box %s (edges)%s" % (path, data.dtype, data.shape, tuple(box), "" if projection is None else ", %s" % projection))


def per_source(values, n, what, default=None):
    """``values`` (None, one value, or a list of one or n) as a list of n"""
    if values is None or isinstance(values, str):
        values = [values if values is not None else default]
    values = list(values)
    if len(values) == 1:
        values = values * n
    if len(values) != n:
        raise ValueError("topography: %d %s for %d sources: give one, or one per source" % (len(values), what, n))
    return [default if v is None else v for v in values]


def read_sources(paths, var=None, proj=None, boxes=None, quantum=None):
    """What topography() samples from the files ``paths`` (a path or a list of them, in order of priority): a Source for one lat-lon
    file, else a SourceList.  ``var`` and ``proj`` (text forms; "latlon" or None: as the file says): one, or one per source; ``boxes``:
    the --source_box of the .npy sources, in their order.  ``quantum``: one per source (None: the source's own), or one value: of the
    one source, or of the float sources of a list (an int16 source keeps its own quantum, else its heights would be rescaled).
    Prints every source's note."""
    paths = [paths] if isinstance(paths, (str, bytes)) or hasattr(paths, "__fspath__") else list(paths)
    n = len(paths)
    var, proj = per_source(var, n, "variables", "elevation"), per_source(proj, n, "projections")
    quanta = list(quantum) if isinstance(quantum, (list, tuple)) else [quantum]
    floats_only = n > 1 and len(quanta) == 1
    quanta = per_source(quanta, n, "quanta")
    boxes = list(boxes or [])
    if boxes and not isinstance(boxes[0], (list, tuple)):
        boxes = [boxes]
    srcs = []
    for path, v, pr, q in zip(paths, var, proj, quanta):
        box = boxes.pop(0) if str(path).endswith(".npy") and boxes else None
        s = read_source(str(path), v, box, None if floats_only else q, pr)
        if floats_only and q is not None and s.data.dtype != np.int16:
            s = s.replace(quantum=q)
        srcs.append(s)
        print(s.note)
    return as_sources(srcs)


def read_source(path, var="elevation", box=None, quantum=None, projection=None):
    """``projection``: a PolarStereo or its text form (PolarStereo.parse), for .npy sources and files without a grid mapping"""
    if isinstance(projection, str) and projection != "latlon":
        projection = PolarStereo.parse(projection)
    if str(path).endswith(".npy"):
        return read_source_npy(path, box, quantum=quantum, projection=None if projection == "latlon" else projection)
    return read_source_nc(path, var, quantum=quantum, projection=projection)


def file_projection(path, var="elevation"):
    """The PolarStereo that read_source_nc would find in the file's own grid mapping of ``var``, from the header alone; None for a
    lat-lon variable, a .npy source, or a file or variable that cannot be read (read_source says why)."""
    if str(path).endswith(".npy"):
        return None
    try:
        h = netcdf3.read_header(str(path))
        return _stereo_mapping(h, h.vars[var])
    except (OSError, KeyError, ValueError):
        return None


# ---- records -------------------------------------------------------------------------------------------------
def has_moments(rec):
    """whether ``rec`` (a record array or its dtype) holds plane records (TOPOG_PLANE_RECORD)"""
    return "sx" in (getattr(rec, "dtype", rec).names or ())


def has_layers(rec):
    """whether ``rec`` (a record array or its dtype) holds merge records (TOPOG_MERGE_RECORD)"""
    return "n_from" in (getattr(rec, "dtype", rec).names or ())


def empty_records(shape, plane=False, merge=False):
    if merge:
        if plane:
            raise ValueError("topography: there are no plane records of layered sources")
        r = np.zeros(shape, dtype=L.TOPOG_MERGE_RECORD)
        for f, v in zip(L.TOPOG_RECORD.names, _EMPTY):
            r[f] = v
        return r
    r = np.empty(shape, dtype=L.TOPOG_PLANE_RECORD if plane else L.TOPOG_RECORD)
    r[...] = _EMPTY_PLANE if plane else _EMPTY
    return r


def merge_into(acc, rec):
    """acc <- the exact combination of acc and rec (same shape and record type): sums of counts (and of the plane moments), min, max,
    the larger R."""
    if has_moments(acc) != has_moments(rec):
        raise ValueError("topography: records with and without plane moments do not combine")
    if has_layers(acc) != has_layers(rec):
        raise ValueError("topography: records of one source and of layers do not combine")
    for f in ("n", "n_missing", "n_wet", "sum", "sumsq", "n_pole", "n_clamped") + (L.TOPOG_MOMENT_FIELDS if has_moments(acc) else ()) + \
            (("n_from",) if has_layers(acc) else ()):
        acc[f] += rec[f]
    acc["min"] = np.minimum(acc["min"], rec["min"])
    acc["max"] = np.maximum(acc["max"], rec["max"])
    acc["R"] = np.maximum(acc["R"], rec["R"])


def assemble(pieces, ny_out, nx_out, plane=None):
    """The records of the whole grid from [(first output row, records (rows x nx_out))]: rows split between two bands combine exactly.
    ``plane``: the record type (default: that of the pieces)."""
    if plane is None:
        plane = bool(pieces) and has_moments(pieces[0][1])
    out = empty_records((ny_out, nx_out), plane, bool(pieces) and has_layers(pieces[0][1]))
    for m0, rec in pieces:
        merge_into(out[m0:m0 + rec.shape[0]], rec)
    return out


def _mul128(a, b):
    """(high, low) uint64 words of the 128-bit product of two uint64 arrays"""
    M = np.uint64(0xFFFFFFFF)
    s32 = np.uint64(32)
    a0, a1, b0, b1 = a & M, a >> s32, b & M, b >> s32
    ll, m1, m2, hh = a0 * b0, a1 * b0, a0 * b1, a1 * b1
    t = (ll >> s32) + (m1 & M) + (m2 & M)
    return hh + (m1 >> s32) + (m2 >> s32) + (t >> s32), (ll & M) | ((t & M) << s32)


def exact_variance_numerator(n, s, ss):
    """(double) of n * ss - s^2, formed exactly in 128-bit integers (n, ss >= 0 and |s| < 2^63; the result is >= 0) and rounded once."""
    n, ss = np.asarray(n, dtype=np.uint64), np.asarray(ss, dtype=np.uint64)
    s = np.abs(np.asarray(s, dtype=np.int64)).astype(np.uint64)
    mul = _mul128
    h1, l1 = mul(n, ss)
    h2, l2 = mul(s, s)
    lo = l1 - l2
    hi = h1 - h2 - (l1 < l2).astype(np.uint64)
    out = lo.astype(np.float64)
    big = hi != 0
    if np.any(big):   # rare (n * ss >= 2^64): Python integers round once
        out[big] = [float((int(h) << 64) | int(lo_)) for h, lo_ in zip(hi[big], lo[big])]
    return out


def exact_centred_moment(n, sab, sa, sb):
    """(double) of n * sab - sa * sb, formed exactly in 128-bit integers (n >= 0, the others signed int64, the result within 2^127) and
    rounded once: exact_variance_numerator for mixed moments, which have a sign."""
    n, sab, sa, sb = (np.atleast_1d(np.asarray(v, dtype=np.int64)) for v in (n, sab, sa, sb))
    n, sab, sa, sb = np.broadcast_arrays(n, sab, sa, sb)
    mag = lambda v: np.abs(v).astype(np.uint64)   # noqa: E731   (|int64 min| wraps to itself and converts rightly)
    one, zero = np.uint64(1), np.uint64(0)

    def signed(h, l, neg):   # the two's-complement 128-bit words of +-(h, l)
        nl = ~l + one
        nh = ~h + (nl == zero).astype(np.uint64)
        return np.where(neg, nh, h), np.where(neg, nl, l)

    h1, l1 = signed(*_mul128(mag(n), mag(sab)), sab < 0)
    h2, l2 = signed(*_mul128(mag(sa), mag(sb)), (sa < 0) != (sb < 0))
    lo = l1 - l2
    hi = h1 - h2 - (l1 < l2).astype(np.uint64)
    neg = (hi >> np.uint64(63)) != zero
    hi, lo = signed(hi, lo, neg)          # the magnitude
    out = lo.astype(np.float64)
    big = hi != zero
    if np.any(big):   # rare (a magnitude of 2^64 or more): Python integers round once
        out[big] = [float((int(h) << 64) | int(lo_)) for h, lo_ in zip(hi[big], lo[big])]
    return np.where(neg, -out, out)


def cell_latitudes(y, cells="model"):
    """latC of every output cell of the stitched supergrid latitudes y ((ny + 1) x (nx + 1)): the centre point of a model cell, the
    mean of the four corners (summed left to right) of a supergrid cell."""
    y = np.asarray(y, dtype=np.float64)
    if cells == "model":
        return np.ascontiguousarray(y[1::2, 1::2])
    with np.errstate(invalid="ignore"):
        return (y[:-1, :-1] + y[:-1, 1:] + y[1:, :-1] + y[1:, 1:]) / 4.0


def plane_fields(rec, quantum, lat_c, dlon, dlat):
    """h2, plane_a, plane_b, slope_east, slope_north and plane_flag of plane records ("Plane-fit topography" of include/ogg_hip.h):
    the centred moments exactly, then the fixed fp64 sequence.  ``lat_c``: cell_latitudes of the cells; dlon, dlat: the raster's."""
    n = rec["n"]
    shape = n.shape
    c = lambda sab, sa, sb: exact_centred_moment(n, rec[sab], rec[sa], rec[sb]).reshape(shape)   # noqa: E731
    Cxx, Cxy, Cyy = c("sxx", "sx", "sx"), c("sxy", "sx", "sy"), c("syy", "sy", "sy")
    Cxq, Cyq, Cqq = c("sxq", "sx", "sum"), c("syq", "sy", "sum"), c("sumsq", "sum", "sum")
    q = float(quantum)
    nf = np.where(n > 0, n, 1).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        d = Cxx * Cyy - Cxy * Cxy
        flag = np.where(n == 0, 0, np.where(rec["n_far"] > 0, 3, np.where((n < 3) | ~(d > 0.0), 2, 1))).astype(np.int8)
        fitted = flag == 1
        dd = np.where(fitted, d, 1.0)
        a = (Cxq * Cyy - Cyq * Cxy) / dd
        b = (Cyq * Cxx - Cxq * Cxy) / dd
        r = Cqq - a * Cxq - b * Cyq
        h2 = np.where(fitted, np.maximum(0.0, r), Cqq) / (nf * nf) * (q * q)
        lat = np.asarray(lat_c, dtype=np.float64)
        if lat.shape != shape:
            raise ValueError("topography: %s cell latitudes for %s records" % (lat.shape, shape))
        east = a * q / (float(dlon) * np.pi / 180.0 * RE * np.cos(lat * np.pi / 180.0))
        north = b * q / (float(dlat) * np.pi / 180.0 * RE)
        polar = ~(np.abs(lat) < 90.0 - L.TOPOG_POLE_EPS)
    return {"h2": np.where(flag == 0, FILL, h2), "plane_a": np.where(fitted, a, FILL), "plane_b": np.where(fitted, b, FILL),
            "slope_east": np.where(fitted & ~polar, east, FILL), "slope_north": np.where(fitted, north, FILL), "plane_flag": flag}


def fields_from_records(rec, quantum, lat_c=None, dlon=None, dlat=None):
    """The outputs of include/ogg_hip.h from the integer records (floats: FILL where n = 0).  Plane records (which then need the
    cells' latitudes ``lat_c`` and the raster's ``dlon``, ``dlat``) add h2, slope_east, slope_north, plane_a, plane_b, plane_flag."""
    n = rec["n"]
    ok = n > 0
    nf = np.where(ok, n, 1).astype(np.float64)
    q = float(quantum)
    with np.errstate(invalid="ignore", divide="ignore"):
        height = rec["sum"].astype(np.float64) / nf * q
        std = np.sqrt(exact_variance_numerator(n, rec["sum"], rec["sumsq"])) / nf * q
        hmin = rec["min"].astype(np.float64) * q
        hmax = rec["max"].astype(np.float64) * q
        wet = rec["n_wet"].astype(np.float64) / nf
    depth = np.maximum(0.0, -height)
    out = {"height": height, "h_std": std, "h_min": hmin, "h_max": hmax, "wet_fraction": wet, "depth": depth}
    for k in out:
        out[k] = np.where(ok, out[k], FILL)
    out["n_samples"] = n.astype(np.int32)
    if has_moments(rec):
        if lat_c is None or dlon is None or dlat is None:
            raise ValueError("topography: the fields of plane records need the cells' latitudes and the raster's dlon and dlat")
        out.update(plane_fields(rec, quantum, lat_c, dlon, dlat))
    return out


def summary_of(rec, plane_flag=None):
    """Counts over the records; with the ``plane_flag`` of plane records also the cells per flag (plane_flag_cells[0 .. 3]) and the
    samples that were far."""
    s = {"n_cells": int(rec.size), "n_pole_cells": int(rec["n_pole"].sum()), "n_clamped_cells": int(rec["n_clamped"].sum()),
         "n_cells_with_missing": int(np.count_nonzero(rec["n_missing"])), "R_max": int(rec["R"].max()) if rec.size else 0,
         "n_samples": int(rec["n"].sum()) + int(rec["n_missing"].sum()), "n_valid_samples": int(rec["n"].sum()),
         "n_empty_cells": int(np.count_nonzero(rec["n"] == 0))}
    if plane_flag is not None:
        s["plane_flag_cells"] = [int(np.count_nonzero(plane_flag == k)) for k in range(4)]
        s["n_far_samples"] = int(rec["n_far"].sum())
    return s


def result(rec, quantum, sea_level, cells, refine, oversample, source=None, lat_c=None):
    """What topography() returns: the output fields, the integer records, and the summary.  Plane records need ``source`` (its dlon
    and dlat) and the cells' latitudes ``lat_c`` (cell_latitudes)."""
    if has_moments(rec) and source is None:
        raise ValueError("topography: the fields of plane records need the source's dlon and dlat")
    out = fields_from_records(rec, quantum, lat_c, *((source.dlon, source.dlat) if has_moments(rec) else ()))
    out["records"] = rec
    out["summary"] = dict(summary_of(rec, out.get("plane_flag")), cells=cells, quantum=float(quantum), sea_level=float(sea_level),
                          refine=None if refine is None else int(refine), oversample=float(oversample))
    if isinstance(source, SourceList):
        nsrc = len(source.sources)
        out["n_from"] = np.ascontiguousarray(np.moveaxis(rec["n_from"][..., :nsrc], -1, 0))   # (nsrc, ny, nx)
        out["source_names"] = list(source.names)
        out["summary"]["sources"] = source.summary()
        out["summary"]["source_descriptions"] = [s.describe() for s in source.sources]
        out["summary"]["n_from"] = [int(v) for v in out["n_from"].reshape(nsrc, -1).sum(axis=1)]
    elif source is not None:
        out["summary"]["source"] = {"shape": list(source.shape), "dtype": str(source.data.dtype), "lon0": source.lon0,
                                    "dlon": source.dlon, "lat0": source.lat0, "dlat": source.dlat, "periodic": bool(source.periodic)}
    return out


def check_args(nyp, nxp, cells, refine, oversample):
    if cells not in ("model", "supergrid"):
        raise ValueError("topography: cells must be 'model' or 'supergrid', not %r" % (cells,))
    ny, nx = nyp - 1, nxp - 1
    if ny < 1 or nx < 1:
        raise ValueError("topography: a grid of %d x %d points has no cells" % (nyp, nxp))
    if cells == "model" and (ny % 2 or nx % 2):
        raise ValueError("topography: model cells are 2 x 2 supergrid cells, but the supergrid has %d x %d cells; generate it with "
                         "--ensure_nj_even, or ask for supergrid cells (--supergrid_cells)" % (ny, nx))
    if refine is not None and not 1 <= int(refine) <= L.TOPOG_MAX_REFINE:
        raise ValueError("topography: refine must be 1 .. %d (%r)" % (L.TOPOG_MAX_REFINE, refine))
    if refine is None and not (oversample > 0 and np.isfinite(oversample)):
        raise ValueError("topography: oversample must be positive (%r)" % (oversample,))


def as_source(source, lon0=None, dlon=None, lat0=None, dlat=None, quantum=None, fill=()):
    if isinstance(source, Source):
        if quantum is not None and float(quantum) != source.quantum:
            source = source.replace(quantum=quantum)
        return source
    if None in (lon0, dlon, lat0, dlat):
        raise ValueError("topography: a raster array needs its box lon0, dlon, lat0, dlat")
    return Source(source, lon0, dlon, lat0, dlat, fill=fill, quantum=quantum)


# ---- host arrays -----------------------------------------------------------------------------------------------
def topography(x, y, source, lon0=None, dlon=None, lat0=None, dlat=None, refine=None, oversample=2.0, quantum=None, sea_level=0.0,
               cells="model", fill=(), plane=False):
    """Topography of a stitched supergrid x, y ((ny + 1) x (nx + 1), degrees) from a raster (a Source, or an int16 / float32 /
    float64 array with its box of cell edges lon0 + is * dlon, lat0 + js * dlat), on one GPU.  ``source`` may also be a list of 1 .. 4
    Sources in order of priority, or a projected Source ("Layered topography" of include/ogg_hip.h: ogg_topog_layers); the result then
    also holds n_from (nsrc x ny x nx, the samples each source gave) and source_names.  One lat-lon Source, alone or in a list, takes
    the single-source entry points as ever.  ``quantum``: the value of one integer
    step (float rasters: default 0.01); ``fill``: raw values that mark missing samples.  A dict of arrays (height, h_std, h_min, h_max,
    wet_fraction, depth, n_samples, and the integer records) and "summary".  ``plane``: plane records (ogg_topog_plane), and with
    them h2, slope_east, slope_north, plane_a, plane_b and plane_flag."""
    src = as_sources(source, lon0=lon0, dlon=dlon, lat0=lat0, dlat=dlat, quantum=quantum, fill=fill)
    layered = isinstance(src, SourceList)
    if layered and plane:
        raise ValueError(NO_PLANE)
    x, y = L.as_f64(x), L.as_f64(y)
    if x.ndim != 2 or y.shape != x.shape:
        raise ValueError("topography: x %s and y %s must be 2-D of one shape" % (x.shape, y.shape))
    nyp, nxp = x.shape
    check_args(nyp, nxp, cells, refine, oversample)
    band = L.TopogBand(nx=nxp - 1, j0=0, n_cell_rows=nyp - 1, cells=L.TOPOG_MODEL_CELLS if cells == "model" else L.TOPOG_SUPERGRID_CELLS,
                       refine=int(refine or 0), oversample=float(oversample))
    band.x, band.y = L.ptr(x), L.ptr(y)
    sh = 1 if cells == "model" else 0
    rec = empty_records(((nyp - 1) >> sh, (nxp - 1) >> sh), plane, layered)
    if layered:
        L.call("ogg_topog_layers", ctypes.byref(band), len(src.sources), src.layers(sea_level), rec.ctypes.data)
    else:
        desc = src.descriptor(sea_level)
        L.call("ogg_topog_plane" if plane else "ogg_topog", ctypes.byref(band), ctypes.byref(desc), rec.ctypes.data)
    return result(rec, src.quantum, sea_level, cells, refine, oversample, src, cell_latitudes(y, cells) if plane else None)


# ---- device arrays ---------------------------------------------------------------------------------------------
def band_records_dev(band, desc, stream, device, plane=False):
    """ogg_topog_band_dev (``plane``: ogg_topog_plane_band_dev) on a descriptor of device pointers: (first output row, records as an
    int64 device tensor rows x n x 7 (plane records: 15), workspace), not synchronised.  ``desc`` an array of layers (the desc of a
    DeviceSourceList): ogg_topog_layers_band_dev, merge records of 11 words."""
    import torch
    rows = int(L.load().ogg_topog_band_out_rows(ctypes.byref(band)))
    nxo = band.nx >> (1 if band.cells == L.TOPOG_MODEL_CELLS else 0)
    layered = isinstance(desc, ctypes.Array)
    if layered and plane:
        raise ValueError(NO_PLANE)
    words = record_words(plane, layered)
    out = torch.empty((rows, nxo, words), dtype=torch.int64, device=device)
    ws_bytes = int(L.load().ogg_topog_workspace_bytes())
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=device)
    if layered:
        L.call("ogg_topog_layers_band_dev", ctypes.byref(band), len(desc), desc, ws.data_ptr(), ws_bytes, out.data_ptr(), stream)
    else:
        L.call("ogg_topog_plane_band_dev" if plane else "ogg_topog_band_dev", ctypes.byref(band), ctypes.byref(desc), ws.data_ptr(),
               ws_bytes, out.data_ptr(), stream)
    return band.j0 >> (1 if band.cells == L.TOPOG_MODEL_CELLS else 0), out, ws


def record_words(plane=False, merge=False):
    """int64 words of a record on the device"""
    return (L.TOPOG_MERGE_RECORD if merge else (L.TOPOG_PLANE_RECORD if plane else L.TOPOG_RECORD)).itemsize // 8


def records_to_host(t):
    """the record array of a device tensor of band_records_dev (any of the record types, told apart by its words)"""
    dtype = {record_words(True): L.TOPOG_PLANE_RECORD, record_words(merge=True): L.TOPOG_MERGE_RECORD}.get(t.shape[2], L.TOPOG_RECORD)
    return np.ascontiguousarray(t.cpu().numpy()).view(dtype).reshape(t.shape[0], t.shape[1])


# ---- files -----------------------------------------------------------------------------------------------------
_VARS = (("height", "m", "mean height of the source over the cell (positive up)"),
         ("depth", "m", "depth of the sea floor, max(0, -height) (positive down)"),
         ("h_std", "m", "standard deviation of the source height over the cell"),
         ("h_min", "m", "smallest source height in the cell"),
         ("h_max", "m", "largest source height in the cell"),
         ("wet_fraction", "1", "fraction of the cell's samples below sea level"))
# written only when the result has them (plane records): name, unit ("m2": the square of the file's unit), long name
_PLANE_VARS = (("h2", "m2", "variance of the source height about the cell's least-squares plane (sub-grid roughness)"),
               ("slope_east", "1", "eastward slope of the cell's least-squares plane (resolved bottom slope)"),
               ("slope_north", "1", "northward slope of the cell's least-squares plane (resolved bottom slope)"))


def write_topog(path, res, units="m"):
    """topog.nc (NetCDF 64-bit offset): dims (ny, nx), the floating outputs as doubles with _FillValue, n_samples as int.  A result of
    layered sources (n_from) adds the dimension nsrc, n_from_source (nsrc, ny, nx) and the global attribute ``sources``: the sources in
    order with their projections; any other result gives the file it always gave."""
    h = res["height"]
    ny, nx = h.shape
    s = res["summary"]
    layered = "n_from" in res
    ds = netcdf3.Dataset(path, ([("nsrc", res["n_from"].shape[0])] if layered else []) + [("ny", ny), ("nx", nx)], global_atts=[
        ("title", "topography by refined sampling of a source raster"),
        ("cells", "MOM6 model (h) cells: 2 x 2 supergrid cells" if s["cells"] == "model" else "supergrid cells"),
        ("quantum", float(s["quantum"])), ("sea_level", float(s["sea_level"])), ("oversample", float(s["oversample"])),
        ("refine", int(s["refine"] or 0))] + ([("sources", "; ".join(s["source_descriptions"]))] if layered else []))
    for name, u, long_name in _VARS:
        ds.def_var(name, netcdf3.NC_DOUBLE, ("ny", "nx"), [("units", units if u == "m" else u), ("long_name", long_name),
                                                            ("_FillValue", FILL)], res[name])
    ds.def_var("n_samples", netcdf3.NC_INT, ("ny", "nx"), [("units", "1"), ("long_name", "number of valid samples in the cell")],
               res["n_samples"])
    if layered:
        ds.def_var("n_from_source", netcdf3.NC_INT, ("nsrc", "ny", "nx"), [("units", "1"), ("long_name", "number of the cell's valid "
                                                                           "samples taken from each source, in the order of the "
                                                                           "global attribute sources")],
                   np.asarray(res["n_from"], dtype=np.int32))
    for name, u, long_name in _PLANE_VARS:
        if name in res:
            ds.def_var(name, netcdf3.NC_DOUBLE, ("ny", "nx"), [("units", units + "2" if u == "m2" else u), ("long_name", long_name),
                                                                ("_FillValue", FILL)], res[name])
    if "plane_flag" in res:
        ds.def_var("plane_flag", netcdf3.NC_BYTE, ("ny", "nx"), [("units", "1"), ("long_name", "plane fit: 0 no valid sample, 1 fitted, "
                                                                  "2 degenerate (h2 about the mean), 3 refused (h2 about the mean)")],
                   np.asarray(res["plane_flag"], dtype=np.int8))
    if "depth_sampled" in res:   # the ocean mask edited depth (ocean_mask.edit_topog): the depth as sampled
        ds.def_var("depth_sampled", netcdf3.NC_DOUBLE, ("ny", "nx"), [("units", units), ("long_name", "depth as sampled, before the "
                                                                                                      "ocean mask"), ("_FillValue", FILL)],
                   res["depth_sampled"])
    ds.write()


def summary_lines(res):
    s = res["summary"]
    h = res["height"]
    ok = res["n_samples"] > 0
    lines = ["   topography: %d %s cells, %d samples (%d valid), R up to %d; %d pole-enclosing, %d clamped, %d with missing samples"
             % (s["n_cells"], s["cells"], s["n_samples"], s["n_valid_samples"], s["R_max"], s["n_pole_cells"], s["n_clamped_cells"],
                s["n_cells_with_missing"])]
    if np.any(ok):
        wet = res["wet_fraction"][ok]
        lines.append("   topography: height %.6g .. %.6g, %d cells all wet, %d all dry, %d partly wet"
                     % (float(h[ok].min()), float(h[ok].max()), int(np.sum(wet == 1.0)), int(np.sum(wet == 0.0)),
                        int(np.sum((wet > 0) & (wet < 1)))))
    if "n_from" in res:
        total = max(1, s["n_valid_samples"])
        lines.append("   topography: valid samples by source: " + ", ".join(
            "%s %.2f %%" % (name, 100.0 * n / total) for name, n in zip(res["source_names"], s["n_from"])))
    if "plane_flag" in res:
        flag = np.asarray(res["plane_flag"])
        lines.append("   topography: plane fit: %d cells fitted, %d degenerate, %d refused (a far or pole sample), %d without a valid sample"
                     % tuple(int(np.count_nonzero(flag == k)) for k in (1, 2, 3, 0)))
        if np.any(ok):
            h2 = np.where(ok, res["h2"], -np.inf)
            j, i = np.unravel_index(int(np.argmax(h2)), h2.shape)
            lines.append("   topography: largest h2 %.6g at cell j=%d, i=%d (plane_flag %d)" % (float(h2[j, i]), j, i, int(flag[j, i])))
    return lines


def main(argv=None):
    p = argparse.ArgumentParser(prog="python -m ocean_model_grid_generator_amd.topography",
                                description="topography of a supergrid file by refined sampling of a source raster")
    p.add_argument("grid", help="ocean_hgrid.nc (NetCDF classic / 64-bit offset)")
    p.add_argument("source", nargs="+", help="source raster: NetCDF classic / 64-bit offset, or .npy with --source_box; up to four, in "
                                             "order of priority (the first with a value for a sample gives it)")
    p.add_argument("-o", "--output", default="topog.nc")
    p.add_argument("--var", action="append", default=None, help="source variable (default elevation); once, or once per source")
    p.add_argument("--source_box", type=float, nargs=4, action="append", default=None, metavar=("LON0", "DLON", "LAT0", "DLAT"),
                   help="cell edges of a .npy source: lon0 + is * dlon, lat0 + js * dlat (a projected source: X0 DX Y0 DY in metres); "
                        "once per .npy source, in their order")
    p.add_argument("--source_proj", action="append", default=None, metavar="PROJ",
                   help="projection of a source that states none: stere:S,lat_ts=-71,lon0=0[,a=..,rf=..], or latlon; once per source "
                        "when given at all")
    p.add_argument("--refine", type=int, default=None, help="R x R samples in every supergrid cell (default: from the cell's spans)")
    p.add_argument("--oversample", type=float, default=2.0)
    p.add_argument("--quantum", type=float, action="append", default=None,
                   help="value of one integer step of a float source (default 0.01); once (with several sources: of the float ones), "
                        "or once per source")
    p.add_argument("--sea_level", type=float, default=0.0)
    p.add_argument("--supergrid_cells", action="store_true", help="one output cell per supergrid cell instead of per model cell")
    p.add_argument("--roughness", action="store_true", help="also fit a plane to every cell's samples: the roughness h2 about it, the "
                                                              "bottom slopes slope_east and slope_north, and plane_flag")
    p.add_argument("--json", default=None, help="write the summary as JSON to this file")
    p.add_argument("--faces", default=None, metavar="FILE",
                   help="also write the face topography of the model grid to FILE (face_topography.py: the sill, the shallowest and "
                        "the mean ridge depth of the lines across every u and v face); one lat-lon source only")
    a = p.parse_args(argv)
    if a.faces and (len(a.source) > 1 or any(pr not in (None, "latlon") for pr in a.source_proj or [])):   # before any file is read
        from . import face_topography as FT
        raise ValueError("--faces: " + FT.NO_FACES)
    src = read_sources(a.source, a.var, a.source_proj, a.source_box, a.quantum)
    if a.faces and isinstance(src, SourceList):   # the file states a projection
        from . import face_topography as FT
        raise ValueError("--faces: " + FT.NO_FACES)
    g = netcdf3.read_doubles(a.grid, names=("x", "y"))
    res = topography(g["x"], g["y"], src, refine=a.refine, oversample=a.oversample, sea_level=a.sea_level,
                     cells="supergrid" if a.supergrid_cells else "model", plane=a.roughness)
    for line in summary_lines(res):
        print(line)
    write_topog(a.output, res)
    if a.faces:
        from . import face_topography as FT
        faces = FT.face_topography(g["x"], g["y"], src, refine=a.refine, oversample=a.oversample, sea_level=a.sea_level)
        for line in FT.summary_lines(faces):
            print(line)
        FT.write_topog_faces(a.faces, faces)
    if a.json:
        with open(a.json, "w") as fh:
            json.dump(res["summary"], fh, indent=1)
    return res


if __name__ == "__main__":
    # run as a script this file is the module __main__; the package's modules (face_topography.py) know the classes of the imported one
    from ocean_model_grid_generator_amd import topography as _module
    _module.main()
    sys.exit(0)
