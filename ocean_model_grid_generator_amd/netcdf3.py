"""Minimal writer for the NetCDF classic format, 64-bit-offset variant (CDF-2) -- what the reference asks netCDF4 for
with format="NETCDF3_64BIT" (OGG:773-779).  Only what write_nc and topog.nc need: fixed-size dimensions, char, numeric
variables, text and single-number attributes, variables laid out in definition order.  The file is a fixed header followed by the
variables' data, big-endian, each padded to 4 bytes, so writing it is a bandwidth-bound stream of the six fields.

Format reference: "The NetCDF Classic Format Specification" (header := magic numrecs dim_list gatt_list var_list).
"""
import struct

import numpy as np

NC_BYTE, NC_CHAR, NC_SHORT, NC_INT, NC_FLOAT, NC_DOUBLE = 1, 2, 3, 4, 5, 6
_NUMPY_TYPE = {NC_BYTE: ">i1", NC_SHORT: ">i2", NC_INT: ">i4", NC_FLOAT: ">f4", NC_DOUBLE: ">f8"}
NC_DIMENSION, NC_VARIABLE, NC_ATTRIBUTE = 0x0A, 0x0B, 0x0C
_ABSENT = struct.pack(">ii", 0, 0)


def _pad4(n):
    return (4 - n % 4) % 4


def _name(s):
    b = s.encode("utf-8")
    return struct.pack(">i", len(b)) + b + b"\0" * _pad4(len(b))


def _att_list(atts):
    if not atts:
        return _ABSENT
    out = struct.pack(">ii", NC_ATTRIBUTE, len(atts))
    for k, v in atts:
        if isinstance(v, (float, np.floating)) or isinstance(v, (int, np.integer)) and not isinstance(v, bool):
            t = NC_DOUBLE if isinstance(v, (float, np.floating)) else NC_INT   # one number: a double or int attribute
            b = np.array([v], dtype=_NUMPY_TYPE[t]).tobytes()
            out += _name(k) + struct.pack(">ii", t, 1) + b + b"\0" * _pad4(len(b))
            continue
        if isinstance(v, np.ndarray):   # several numbers (CF's flag_values): int32 or float64
            t = NC_DOUBLE if v.dtype.kind == "f" else NC_INT
            b = v.reshape(-1).astype(_NUMPY_TYPE[t]).tobytes()
            out += _name(k) + struct.pack(">ii", t, v.size) + b + b"\0" * _pad4(len(b))
            continue
        b = v if isinstance(v, bytes) else str(v).encode("utf-8")
        out += _name(k) + struct.pack(">ii", NC_CHAR, len(b)) + b + b"\0" * _pad4(len(b))
    return out


class Dataset(object):
    """dims: [(name, length)], in order.  Variables are added with def_var (host array) or decl_var (layout only: the data is
    streamed into the file by the caller at var_begin(name)); write() writes header and host arrays, write_header() the header
    alone.  ``record_dim`` (opt-in): the name of one dimension written as the unlimited (record) dimension; the variables whose first
    dimension it is are record variables, stored after the fixed-size ones one record at a time (write() only)."""

    def __init__(self, path, dims, global_atts=(), record_dim=None):
        self.path = path
        self.dims = list(dims)
        self.gatts = list(global_atts)
        self.vars = []  # (name, nc_type, dim names, attrs, array or None)
        self._layout = None
        if record_dim is not None and record_dim not in dict(self.dims):
            raise ValueError("record dimension %s is not one of the dimensions" % record_dim)
        self.record_dim = record_dim

    def _is_record(self, v):
        return self.record_dim is not None and len(v[2]) > 0 and v[2][0] == self.record_dim

    def _shape(self, dim_names):
        return tuple(dict(self.dims)[d] for d in dim_names)

    def def_var(self, name, nc_type, dim_names, atts, data):
        shape = self._shape(dim_names)
        data = np.asarray(data)
        if tuple(data.shape) != shape:
            raise ValueError("variable %s: data shape %s does not match dimensions %s" % (name, data.shape, shape))
        self.vars.append((name, nc_type, tuple(dim_names), list(atts), data))
        self._layout = None

    def decl_var(self, name, nc_type, dim_names, atts):
        self.vars.append((name, nc_type, tuple(dim_names), list(atts), None))
        self._layout = None

    def layout(self):
        """(header bytes, [begin offset of each variable], [byte size of each variable], total file size)"""
        if self._layout is not None:
            return self._layout
        if self.record_dim is not None:
            self._layout = self._record_layout()
            return self._layout
        dimid = {n: k for k, (n, _) in enumerate(self.dims)}
        esize = {NC_CHAR: 1, NC_BYTE: 1, NC_SHORT: 2, NC_INT: 4, NC_FLOAT: 4, NC_DOUBLE: 8}

        def var_header(name, nc_type, dnames, atts, nbytes, begin):
            vsize = nbytes + _pad4(nbytes)
            if vsize > 2 ** 32 - 4:
                vsize = 2 ** 32 - 1
            h = _name(name) + struct.pack(">i", len(dnames)) + b"".join(struct.pack(">i", dimid[d]) for d in dnames)
            return h + _att_list(atts) + struct.pack(">iI", nc_type, vsize) + struct.pack(">q", begin)

        head = b"CDF\x02" + struct.pack(">i", 0)
        head += struct.pack(">ii", NC_DIMENSION, len(self.dims)) + b"".join(_name(n) + struct.pack(">i", l) for n, l in self.dims)
        head += _att_list(self.gatts)
        sizes = [int(np.prod(self._shape(v[2]), dtype=np.int64)) * esize[v[1]] for v in self.vars]
        # header length does not depend on the begin values (fixed-width), so compute it with zeros first
        var_list = struct.pack(">ii", NC_VARIABLE, len(self.vars)) if self.vars else _ABSENT
        probe = head + var_list + b"".join(var_header(v[0], v[1], v[2], v[3], s, 0) for v, s in zip(self.vars, sizes))
        begin = len(probe)
        body = b""
        begins = []
        for v, s in zip(self.vars, sizes):
            begins.append(begin)
            body += var_header(v[0], v[1], v[2], v[3], s, begin)
            begin += s + _pad4(s)
        self._layout = (head + var_list + body, begins, sizes, begin)
        return self._layout

    def _record_layout(self):
        """layout() with a record dimension: for a record variable the size is that of one record (padded to 4 bytes unless it is the
        only record variable) and the begin that of its slab in record 0; the file's records follow the fixed-size data."""
        dimid = {n: k for k, (n, _) in enumerate(self.dims)}
        esize = {NC_CHAR: 1, NC_BYTE: 1, NC_SHORT: 2, NC_INT: 4, NC_FLOAT: 4, NC_DOUBLE: 8}
        nrec = dict(self.dims)[self.record_dim]
        recs = [v for v in self.vars if self._is_record(v)]

        def size(v):
            shape = self._shape(v[2][1:] if self._is_record(v) else v[2])
            n = int(np.prod(shape, dtype=np.int64)) * esize[v[1]]
            return n + (_pad4(n) if not (self._is_record(v) and len(recs) == 1) else 0)

        def var_header(name, nc_type, dnames, atts, vsize, begin):
            h = _name(name) + struct.pack(">i", len(dnames)) + b"".join(struct.pack(">i", dimid[d]) for d in dnames)
            return h + _att_list(atts) + struct.pack(">iI", nc_type, min(vsize, 2 ** 32 - 1)) + struct.pack(">q", begin)

        head = b"CDF\x02" + struct.pack(">i", nrec)
        head += struct.pack(">ii", NC_DIMENSION, len(self.dims)) + b"".join(
            _name(n) + struct.pack(">i", 0 if n == self.record_dim else l) for n, l in self.dims)
        head += _att_list(self.gatts)
        sizes = [size(v) for v in self.vars]
        var_list = struct.pack(">ii", NC_VARIABLE, len(self.vars)) if self.vars else _ABSENT
        begin = len(head + var_list + b"".join(var_header(v[0], v[1], v[2], v[3], s, 0) for v, s in zip(self.vars, sizes)))
        begins = [0] * len(self.vars)
        for k, v in enumerate(self.vars):
            if not self._is_record(v):
                begins[k] = begin
                begin += sizes[k]
        recsize = 0
        for k, v in enumerate(self.vars):
            if self._is_record(v):
                begins[k] = begin + recsize
                recsize += sizes[k]
        body = b"".join(var_header(v[0], v[1], v[2], v[3], s, b) for v, s, b in zip(self.vars, sizes, begins))
        return (head + var_list + body, begins, sizes, begin + nrec * recsize)

    def var_begin(self, name):
        _, begins, _, _ = self.layout()
        return begins[[v[0] for v in self.vars].index(name)]

    def write_header(self, fd):
        """Header at offset 0 of the open file descriptor, file extended to its final size (the padding bytes are zeros)."""
        import os
        header, _, _, total = self.layout()
        os.ftruncate(fd, total)
        os.pwrite(fd, header, 0)

    def write(self, chunk_rows=256):
        if self.record_dim is not None:
            return self._write_records()
        header, begins, sizes, _ = self.layout()
        with open(self.path, "wb") as f:
            f.write(header)
            for v, s, b in zip(self.vars, sizes, begins):
                assert f.tell() == b
                data = v[4]
                if data is None:
                    raise ValueError("variable %s was declared without data: use write_header() and stream it" % v[0])
                if v[1] == NC_CHAR:
                    f.write(np.ascontiguousarray(data).tobytes())
                else:
                    flat = data.reshape(-1, data.shape[-1]) if data.ndim > 1 else data.reshape(1, -1)
                    for r0 in range(0, flat.shape[0], chunk_rows):
                        f.write(np.ascontiguousarray(flat[r0:r0 + chunk_rows]).astype(_NUMPY_TYPE[v[1]]).tobytes())
                f.write(b"\0" * _pad4(s))


    def _write_records(self):
        header, begins, sizes, total = self.layout()
        for v in self.vars:
            if v[4] is None:
                raise ValueError("variable %s was declared without data: a file with a record dimension is written whole" % v[0])
        with open(self.path, "wb") as f:
            f.write(header)
            for v, s, b in zip(self.vars, sizes, begins):
                if self._is_record(v):
                    continue
                assert f.tell() == b
                raw = np.ascontiguousarray(v[4]).astype(_NUMPY_TYPE.get(v[1], "S1")).tobytes()
                f.write(raw + b"\0" * (s - len(raw)))
            recs = [(v, s) for v, s in zip(self.vars, sizes) if self._is_record(v)]
            for r in range(dict(self.dims)[self.record_dim]):
                for v, s in recs:
                    raw = np.ascontiguousarray(v[4][r]).astype(_NUMPY_TYPE.get(v[1], "S1")).tobytes()
                    f.write(raw + b"\0" * (s - len(raw)))
            assert f.tell() == total


# ---- reader ------------------------------------------------------------------------------------------------------
_TYPE_SIZE = {1: 1, 2: 1, 3: 2, 4: 4, 5: 4, 6: 8}   # NC_BYTE, NC_CHAR, NC_SHORT, NC_INT, NC_FLOAT, NC_DOUBLE


class Variable(object):
    def __init__(self, name, nc_type, shape, begin, is_record, atts=None):
        self.name, self.nc_type, self.shape, self.begin, self.is_record = name, nc_type, tuple(shape), begin, is_record
        self.atts = atts if atts is not None else {}   # name -> str (char attribute) or 1-D numpy array
        self.dims = ()                                  # dimension names


NUMPY_DTYPE = {t: np.dtype(d) for t, d in _NUMPY_TYPE.items()}   # NetCDF type -> big-endian numpy dtype of its data


class Header(object):
    """What read_header() finds: version (1 or 2), dims [(name, length)], vars {name: Variable}, global attributes gatts {name:
    str or 1-D numpy array}."""

    def __init__(self, version, dims, vars, gatts=None):
        self.version, self.dims, self.vars = version, dims, vars
        self.gatts = gatts if gatts is not None else {}


def read_header(path):
    """Header of a NetCDF classic (CDF-1) or 64-bit-offset (CDF-2) file.  CDF-5 and NetCDF-4 / HDF5 files are refused."""
    with open(path, "rb") as f:
        head = f.read(4)
        if head[:3] == b"CDF" and head[3:4] == b"\x05":
            raise ValueError("%s: NetCDF CDF-5 (64-bit data) is not supported; write the grid as NETCDF3_64BIT" % path)
        if head[:4] == b"\x89HDF":
            raise ValueError("%s: NetCDF-4 / HDF5 is not supported; write the grid as NETCDF3_64BIT" % path)
        if head[:3] != b"CDF" or head[3:4] not in (b"\x01", b"\x02"):
            raise ValueError("%s: not a NetCDF classic file" % path)
        version = head[3]
        data = head + f.read(1 << 20)
        while True:   # headers of grid files are small; read more only if one is not
            try:
                return _parse_header(path, data, version)
            except IndexError:
                more = f.read(len(data))
                if not more:
                    raise ValueError("%s: truncated NetCDF header" % path)
                data += more


def _parse_header(path, data, version):
    pos = [4]

    def take(n):
        if pos[0] + n > len(data):
            raise IndexError
        b = data[pos[0]:pos[0] + n]
        pos[0] += n
        return b

    def i32():
        return struct.unpack(">i", take(4))[0]

    def name():
        n = i32()
        s = take(n).decode("utf-8")
        take(_pad4(n))
        return s

    def atts():
        tag, n = i32(), i32()
        if tag not in (0, NC_ATTRIBUTE):
            raise ValueError("%s: bad attribute list" % path)
        out = {}
        for _ in range(n):
            k = name()
            t, m = i32(), i32()
            if t not in _TYPE_SIZE:
                raise ValueError("%s: attribute %s has NetCDF type %d (not a classic type)" % (path, k, t))
            nb = m * _TYPE_SIZE[t]
            raw = take(nb + _pad4(nb))[:nb]
            out[k] = raw.decode("utf-8", "replace") if t == NC_CHAR else np.frombuffer(raw, dtype=_NUMPY_TYPE[t]).astype(
                _NUMPY_TYPE[t].replace(">", "="))
        return out

    numrecs = i32()
    tag, ndims = i32(), i32()
    if tag not in (0, NC_DIMENSION):
        raise ValueError("%s: bad dimension list" % path)
    dims = [(name(), i32()) for _ in range(ndims)]
    gatts = atts()
    tag, nvars = i32(), i32()
    if tag not in (0, NC_VARIABLE):
        raise ValueError("%s: bad variable list" % path)
    out = {}
    for _ in range(nvars):
        vname = name()
        ids = [i32() for _ in range(i32())]
        vatts = atts()
        nc_type = i32()
        take(4)   # vsize
        begin = struct.unpack(">q" if version == 2 else ">i", take(8 if version == 2 else 4))[0]
        is_rec = bool(ids) and dims[ids[0]][1] == 0
        shape = [numrecs if (k == 0 and is_rec) else dims[d][1] for k, d in enumerate(ids)]
        out[vname] = Variable(vname, nc_type, shape, begin, is_rec, vatts)
        out[vname].dims = tuple(dims[d][0] for d in ids)
    return Header(version, dims, out, gatts)


def read_var_bytes(path, header, name, dtype=NC_DOUBLE):
    """The raw (big-endian) bytes of a fixed-size variable."""
    if name not in header.vars:
        raise KeyError("%s: no variable %r" % (path, name))
    v = header.vars[name]
    if v.is_record:
        raise ValueError("%s: %s is a record variable (only fixed-size variables are read)" % (path, name))
    if v.nc_type != dtype:
        raise ValueError("%s: %s has NetCDF type %d, expected %d" % (path, name, v.nc_type, dtype))
    n = int(np.prod(v.shape, dtype=np.int64)) * _TYPE_SIZE[v.nc_type]
    with open(path, "rb") as f:
        f.seek(v.begin)
        b = f.read(n)
    if len(b) != n:
        raise ValueError("%s: %s is truncated" % (path, name))
    return b


def read_record_var_bytes(path, header, name, dtype=NC_DOUBLE):
    """The raw (big-endian) bytes of a record variable, its records one after the other (the file interleaves them with the
    other record variables: one record of every record variable after the other, each slab padded to 4 bytes unless the file has a
    single record variable)."""
    if name not in header.vars:
        raise KeyError("%s: no variable %r" % (path, name))
    v = header.vars[name]
    if not v.is_record:
        raise ValueError("%s: %s is not a record variable" % (path, name))
    if v.nc_type != dtype:
        raise ValueError("%s: %s has NetCDF type %d, expected %d" % (path, name, v.nc_type, dtype))
    recs = [u for u in header.vars.values() if u.is_record]

    def slab(u):
        n = int(np.prod(u.shape[1:], dtype=np.int64)) * _TYPE_SIZE[u.nc_type]
        return n + (_pad4(n) if len(recs) > 1 else 0)
    recsize = sum(slab(u) for u in recs)
    n = int(np.prod(v.shape[1:], dtype=np.int64)) * _TYPE_SIZE[v.nc_type]
    out = []
    with open(path, "rb") as f:
        for r in range(v.shape[0]):
            f.seek(v.begin + r * recsize)
            b = f.read(n)
            if len(b) != n:
                raise ValueError("%s: %s is truncated at record %d" % (path, name, r))
            out.append(b)
    return b"".join(out)


def read_doubles(path, names=("x", "y", "dx", "dy", "area")):
    """{name: host float64 array} of fixed-size double variables (host byte swap; the GPU checker swaps on the device)."""
    h = read_header(path)
    return {n: np.frombuffer(read_var_bytes(path, h, n), dtype=">f8").astype(np.float64).reshape(h.vars[n].shape) for n in names}
