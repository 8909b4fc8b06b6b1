"""Device memory whose surroundings are known: an arena that hands tensors out flush against guard bands of a known byte pattern, and
a context that makes the package's own allocations come from it.

The wrappers of ocean_model_grid_generator_amd allocate every output and workspace with torch.empty / torch.zeros, which the caching
allocator rounds up: a kernel that writes a few elements past an end, or reads a word no step of this call has written, shows nowhere.
Under ``guarded`` every such allocation is an exact-size view into one Arena:

* its absolute address is a multiple of 256 (what torch itself gives), its last byte lies flush against the guard (the size is not
  rounded up), and at least ``guard`` bytes of pattern lie on either side;
* memory is bumped and never reused until the next reset(), so a late write to a tensor that was dropped still lands in the arena;
* reset("ff") makes every byte 0xFF (doubles and floats read as NaN, int32 as -1, flag bytes as 255), reset(("random", seed)) makes
  them seeded random bytes: a result that depends on what its torch.empty memory held differs between the two; reset("00") makes every
  byte 0 (tests/test_gpu_streams.py: a step that runs before the step it depends on reads counts and indices of 0, never an address
  out of range);
* check() lists every changed guard byte with the tensor it belongs to.

The guard is 64 KiB on each side: a condition, not a measurement.  It covers one whole extra row of the widest small input used in
the suite (the 8000-node ``over_lds`` source, 32 000 bytes of float32) and any tail of a 256-thread workgroup storing 16 bytes per lane.

Sizes (measured by tests/test_gpu_extents.py on an MI355X, which prints them): its largest case has 117 015 180 bytes handed out
(used()) and takes 120 888 288 bytes of the arena with its guard bands (used(guards=True)); its arena is twice the latter,
241 776 576 bytes, and stands three times in device memory (the bytes, their pristine copy, the guard map).
"""
import contextlib
import os
import sys

import numpy as np
import torch

GUARD = 65536
ALIGN = 256
BLOCK = 16 << 20     # the pattern is laid down in blocks of this many bytes
_HERE = os.path.abspath(__file__)
# the real functions, whatever is patched in when a method of this module runs
_REAL = {"empty": torch.empty, "zeros": torch.zeros, "empty_like": torch.empty_like, "zeros_like": torch.zeros_like, "tensor": torch.tensor,
         "cat": torch.cat, "stack": torch.stack, "to": torch.Tensor.to, "contiguous": torch.Tensor.contiguous,
         "clone": torch.Tensor.clone}


def _caller():
    """file:line of the first frame outside this module (and outside contextlib)"""
    f = sys._getframe(1)
    while f is not None:
        name = f.f_code.co_filename
        if os.path.abspath(name) != _HERE and os.path.basename(name) != "contextlib.py":
            return "%s:%d" % (os.path.basename(name), f.f_lineno)
        f = f.f_back
    return "?"


def _same_device(arena_dev, d):
    d = torch.device(d)
    if d.type != arena_dev.type:
        return False
    if d.type != "cuda":
        return True
    index = d.index if d.index is not None else torch.cuda.current_device()
    return index == (arena_dev.index if arena_dev.index is not None else torch.cuda.current_device())


class ArenaFull(RuntimeError):
    pass


class Arena(object):
    """Arena(device, nbytes, guard=65536): ``nbytes`` of uint8 memory (buf), a pristine copy of it and a boolean map of which bytes
    are guard (is_guard; every byte that take() has not handed out as part of a tensor)."""

    def __init__(self, device, nbytes, guard=GUARD):
        self.device = torch.device(device)
        self.guard, self.nbytes = int(guard), int(nbytes)
        raw = _REAL["empty"](self.nbytes + ALIGN, dtype=torch.uint8, device=self.device)
        shift = (-raw.data_ptr()) % ALIGN             # offsets into buf that are multiples of 256 are absolute multiples of 256
        self._raw = raw
        self.buf = raw[shift:shift + self.nbytes]
        self.pristine = _REAL["empty"](self.nbytes, dtype=torch.uint8, device=self.device)
        self.is_guard = _REAL["empty"](self.nbytes, dtype=torch.bool, device=self.device)
        self.peak = self.peak_count = 0
        self.reset("ff")

    def reset(self, pattern="ff"):
        """Refill: "ff" (every byte 0xFF), "00" (every byte 0) or ("random", seed) (seeded random bytes); everything handed out before
        is forgotten.  (The pattern is laid down as take() advances, _fill_to: the first block now.)"""
        if pattern not in ("ff", "00") and not (isinstance(pattern, tuple) and len(pattern) == 2 and pattern[0] == "random"):
            raise ValueError("pattern: 'ff', '00' or ('random', seed), not %r" % (pattern,))
        self.pattern = pattern
        self.records = []            # (owner, start, end, row bytes, stride bytes): the tensor is buf[start:end], padding included
        self._cursor = self._handed = self._filled = 0
        self._fill_to(1)

    def _fill_to(self, top):
        """The pattern goes in block by block as take() advances (a reset does not pay for the part of the arena no case reaches);
        nothing before ``_filled`` is ever handed out or checked.  A random block depends on the seed and the block alone."""
        while self._filled < min(top, self.nbytes):
            lo = self._filled
            hi = min(lo + BLOCK, self.nbytes)
            if self.pattern in ("ff", "00"):
                self.buf[lo:hi].fill_(0xFF if self.pattern == "ff" else 0)
            else:
                g = torch.Generator(device=self.device).manual_seed(int(self.pattern[1]) * 1000003 + lo // BLOCK)
                self.buf[lo:hi].random_(0, 256, generator=g)
            self.pristine[lo:hi].copy_(self.buf[lo:hi])
            self.is_guard[lo:hi].fill_(True)
            self._filled = hi

    def take(self, shape, dtype, ld=None, owner=None):
        """A view of ``shape`` and ``dtype`` out of fresh arena memory.  With ``ld`` the view is (rows, cols) with a row stride of ld
        elements; its padding columns keep the pattern and count as guard (for inputs only: an output has no business there)."""
        if isinstance(shape, (int, np.integer)):
            shape = (int(shape),)
        shape = tuple(int(s) for s in shape)
        if any(s < 0 for s in shape):
            raise ValueError("negative dimension in %r" % (shape,))
        item = _REAL["empty"](0, dtype=dtype).element_size()
        if ld is None:
            n = int(np.prod(shape, dtype=np.int64)) if shape else 1
            row = stride = n * item
            nbytes = n * item
        else:
            if len(shape) != 2 or ld < shape[1]:
                raise ValueError("ld needs a (rows, cols) shape with cols <= ld, not %r with ld %r" % (shape, ld))
            rows, cols = shape
            row, stride = cols * item, int(ld) * item
            nbytes = ((rows - 1) * stride + row) if rows and cols else 0
        start = -(-(self._cursor + self.guard) // ALIGN) * ALIGN
        end = start + nbytes
        if end + self.guard > self.nbytes:
            raise ArenaFull("arena of %d bytes is full: %d used, %d more asked for by %s" % (self.nbytes, self._cursor, nbytes, owner or _caller()))
        self._fill_to(end + self.guard)
        self._cursor = end
        self._handed += nbytes if ld is None else shape[0] * row
        self.records.append((owner or _caller(), start, end, row, stride))
        self.peak, self.peak_count = max(self.peak, end + self.guard), max(self.peak_count, len(self.records))
        region = self.buf[start:end]
        g = self.is_guard[start:end]
        if ld is None:
            g.fill_(False)
            return region.view(dtype).view(shape)
        if nbytes == 0:
            return region.view(dtype).view(shape)
        rows = shape[0]
        if rows > 1:
            g[:(rows - 1) * stride].view(rows - 1, stride)[:, :row] = False
        g[(rows - 1) * stride:] = False
        return torch.as_strided(region.view(dtype), shape, (int(ld), 1))

    def used(self, guards=False):
        """The bytes handed out since the last reset (padding columns not counted); with ``guards`` the bytes of the arena they took,
        with their guard bands and alignment."""
        if not guards:
            return self._handed
        return self._cursor + self.guard if self.records else 0

    def count(self):
        return len(self.records)

    def check(self):
        """Every changed guard byte as (owner, side, offset), in address order.  side "before": the byte lies ``offset`` bytes before
        the owner's first byte (1 is the byte just before it); "after": ``offset`` bytes after its last byte (1 is the byte just after
        it); "padding": in a padding column, ``offset`` bytes from the owner's first byte.  A byte between two tensors goes to the
        nearer one.  A byte changed with no tensor handed out has the owner None and its arena offset."""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        top = min(self.nbytes, self._cursor + self.guard) if self.records else self._filled
        bad = ((self.buf[:top] != self.pristine[:top]) & self.is_guard[:top]).nonzero().view(-1).cpu().numpy()
        if bad.size == 0:
            return []
        if not self.records:
            return [(None, "after", int(o)) for o in bad]
        starts = np.array([r[1] for r in self.records], dtype=np.int64)
        ends = np.array([r[2] for r in self.records], dtype=np.int64)
        out = []
        k = np.searchsorted(starts, bad, side="right") - 1     # the last tensor that starts at or before the byte
        for o, i in zip(bad.tolist(), k.tolist()):
            if i >= 0 and o < ends[i]:
                out.append((self.records[i][0], "padding", o - int(starts[i])))
            elif i < 0 or (i + 1 < len(starts) and starts[i + 1] - o <= o - ends[i] + 1):
                out.append((self.records[i + 1][0], "before", int(starts[i + 1]) - o))
            else:
                out.append((self.records[i][0], "after", o - int(ends[i]) + 1))
        return out


def _size_of(args, kwargs):
    """the size of torch.empty / torch.zeros given as varargs, a tuple, a list, a torch.Size or size="""
    if "size" in kwargs:
        args = (kwargs.pop("size"),)
    if len(args) == 1 and isinstance(args[0], (tuple, list, torch.Size)):
        return tuple(int(s) for s in args[0])
    return tuple(int(s) for s in args)


_PLAIN = ("size", "dtype","device", "requires_grad", "pin_memory", "layout", "memory_format")


@contextlib.contextmanager
def guarded(monkeypatch, arena):
    """Within the context torch.empty, torch.zeros, torch.empty_like and torch.zeros_like on the arena's device give arena views, and
    so do the other forms the package allocates with: torch.tensor(device=), torch.cat, torch.stack, and Tensor.to / .contiguous /
    .clone where they make a new tensor there (the result is copied into an arena view).  Anything on another device, on the CPU
    while the arena is elsewhere, or pinned goes to the real function.  ``arena.log`` counts the allocations by form.  On leaving,
    the real functions are back."""
    log = arena.log = {}

    def mine(device, kwargs=None):
        if kwargs is not None and (kwargs.get("pin_memory") or kwargs.get("out") is not None or set(kwargs) - set(_PLAIN)):
            return False
        if kwargs is not None and kwargs.get("layout", torch.strided) is not torch.strided:
            return False
        if device is None:
            device = torch.get_default_device() if hasattr(torch, "get_default_device") else "cpu"
        return _same_device(arena.device, device)

    def fresh(form, shape, dtype):
        log[form] = log.get(form, 0) + 1
        return arena.take(shape, dtype or torch.get_default_dtype(), owner=_caller())

    def rehome(form, t, src=()):
        """t in arena memory, if it is a new tensor on the arena's device (not one of ``src``, nor a view of one)"""
        if not isinstance(t, torch.Tensor) or not mine(t.device) or t.layout is not torch.strided:
            return t
        if any(isinstance(s, torch.Tensor) and s.device == t.device and s.numel() and t.numel()
               and s.untyped_storage().data_ptr() == t.untyped_storage().data_ptr() for s in src):
            return t
        if not t.is_contiguous():
            return t
        v = fresh(form, t.shape, t.dtype)
        v.copy_(t)
        return v

    def empty(*args, **kwargs):
        if not mine(kwargs.get("device"), kwargs):
            return _REAL["empty"](*args, **kwargs)
        return fresh("empty", _size_of(args, kwargs), kwargs.get("dtype"))

    def zeros(*args, **kwargs):
        if not mine(kwargs.get("device"), kwargs):
            return _REAL["zeros"](*args, **kwargs)
        return fresh("zeros", _size_of(args, kwargs), kwargs.get("dtype")).zero_()

    def empty_like(t, **kwargs):
        if not mine(kwargs.get("device") or t.device, kwargs):
            return _REAL["empty_like"](t, **kwargs)
        return fresh("empty_like", t.shape, kwargs.get("dtype") or t.dtype)

    def zeros_like(t, **kwargs):
        if not mine(kwargs.get("device") or t.device, kwargs):
            return _REAL["zeros_like"](t, **kwargs)
        return fresh("zeros_like", t.shape, kwargs.get("dtype") or t.dtype).zero_()

    def tensor(*args, **kwargs):
        return rehome("tensor", _REAL["tensor"](*args, **kwargs))

    def cat(tensors, *args, **kwargs):
        tensors = list(tensors)
        return rehome("cat", _REAL["cat"](tensors, *args, **kwargs), tensors)

    def stack(tensors, *args, **kwargs):
        tensors = list(tensors)
        return rehome("stack", _REAL["stack"](tensors, *args, **kwargs), tensors)

    def to(self, *args, **kwargs):
        return rehome("to", _REAL["to"](self, *args, **kwargs), (self,))

    def contiguous(self, *args, **kwargs):
        return rehome("contiguous", _REAL["contiguous"](self, *args, **kwargs), (self,))

    def clone(self, *args, **kwargs):
        return rehome("clone", _REAL["clone"](self, *args, **kwargs))

    with monkeypatch.context() as m:
        for name, fn in (("empty", empty), ("zeros", zeros), ("empty_like", empty_like), ("zeros_like", zeros_like), ("tensor", tensor),
                         ("cat", cat), ("stack", stack)):
            m.setattr(torch, name, fn)
        for name, fn in (("to", to), ("contiguous", contiguous), ("clone", clone)):
            m.setattr(torch.Tensor, name, fn)
        yield arena
