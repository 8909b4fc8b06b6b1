"""tests/guarded_memory.py proved on the CPU (an arena on device="cpu"): planted bytes are found with their owner, side and offset,
writes inside a tensor are not, the patched allocators take every size spelling and pass other devices through, a read of
uninitialised memory shows as a difference between the two patterns, and the real functions come back."""
import numpy as np
import pytest
import torch

import guarded_memory as gm

SMALL = 4096   # a guard that keeps these arenas small; the default is gm.GUARD


def arena(nbytes=1 << 16, guard=SMALL):
    return gm.Arena("cpu", nbytes, guard=guard)


def test_default_guard_is_64_kib():
    assert gm.GUARD == 65536
    a = gm.Arena("cpu", 4 * gm.GUARD)
    assert a.guard == 65536 and a.buf.dtype == torch.uint8 and a.pristine.dtype == torch.uint8 and a.is_guard.dtype == torch.bool
    assert a.buf.numel() == a.pristine.numel() == a.is_guard.numel() == 4 * gm.GUARD


@pytest.mark.parametrize("shape, dtype", [((7,), torch.float64), ((3, 5), torch.float32), ((13,), torch.uint8), ((1,), torch.int32),
                                          ((0,), torch.float64), ((2, 0, 3), torch.int64)])
def test_take_is_aligned_exact_and_guarded(shape, dtype):
    a = arena()
    first = a.take(5, torch.uint8)
    t = a.take(shape, dtype)
    assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous()
    assert t.data_ptr() % 256 == 0 and first.data_ptr() % 256 == 0
    nbytes = t.numel() * t.element_size()
    start = t.data_ptr() - a.buf.data_ptr() if nbytes else a.records[-1][1]
    assert a.records[-1][1:3] == (start, start + nbytes)                    # the size is not rounded up
    g = a.is_guard.numpy()
    assert not g[start:start + nbytes].any()
    assert g[start - SMALL:start].all() and g[start + nbytes:start + nbytes + SMALL].all()   # at least ``guard`` bytes on either side
    assert start - SMALL >= a.records[0][2]                                 # and none of them is the neighbour's
    assert a.used() == 5 + nbytes and a.count() == 2
    assert a.used(guards=True) == start + nbytes + SMALL
    assert a.check() == []


def test_memory_is_bumped_not_reused_until_reset():
    a = arena()
    p = [a.take(16, torch.uint8).data_ptr() for _ in range(4)]
    assert len(set(p)) == 4 and p == sorted(p)
    a.reset("ff")
    assert a.used() == 0 and a.count() == 0 and a.take(16, torch.uint8).data_ptr() == p[0]
    with pytest.raises(gm.ArenaFull):
        a.take(1 << 16, torch.uint8)


def test_patterns():
    a = arena()
    a.reset("ff")
    assert np.isnan(a.take(3, torch.float64).numpy()).all() and np.isnan(a.take(3, torch.float32).numpy()).all()
    assert a.take(3, torch.int32).tolist() == [-1] * 3 and a.take(3, torch.uint8).tolist() == [255] * 3
    a.reset("00")
    assert a.take(3, torch.float64).tolist() == [0.0] * 3 and a.take(3, torch.int64).tolist() == [0] * 3 and a.check() == []
    assert not a.buf.numpy().any() and not a.pristine.numpy().any()
    a.reset(("random", 3))
    one = a.buf.numpy().copy()
    assert len(np.unique(one)) == 256
    a.reset(("random", 3))
    assert np.array_equal(one, a.buf.numpy()) and np.array_equal(one, a.pristine.numpy())
    a.reset(("random", 4))
    assert not np.array_equal(one, a.buf.numpy())
    with pytest.raises(ValueError):
        a.reset("zero")


def test_planted_bytes_are_reported_with_owner_side_and_offset():
    a = arena()
    a.take(11, torch.float64, owner="first")
    t = a.take((3, 5), torch.float32, owner="second")
    a.take(2, torch.int32, owner="third")
    flat = a.buf
    start = t.data_ptr() - a.buf.data_ptr()
    t.fill_(1.5)                                        # a write inside the tensor is not reported
    assert a.check() == []
    flat[start - 1] ^= 0x5A
    assert a.check() == [("second", "before", 1)]
    flat[start + 60] ^= 0x5A
    assert a.check() == [("second", "before", 1), ("second", "after", 1)]
    flat[start + 60 + 7] ^= 0x5A
    assert a.check() == [("second", "before", 1), ("second", "after", 1), ("second", "after", 8)]
    third = a.records[2][1]
    flat[third - 3] ^= 1                                # nearer to "third" than to "second"
    assert a.check()[-1] == ("third", "before", 3)
    flat[third + 8 + SMALL - 1] ^= 1                    # the last guard byte of the last tensor
    assert a.check()[-1] == ("third", "after", SMALL)
    assert t.tolist() == [[1.5] * 5] * 3


def test_padding_columns_are_guard():
    a = arena()
    t = a.take((3, 5), torch.float64, ld=7, owner="strided")
    assert tuple(t.shape) == (3, 5) and t.stride() == (7, 1) and t.data_ptr() % 256 == 0
    start = t.data_ptr() - a.buf.data_ptr()
    assert a.records[0][1:3] == (start, start + (2 * 7 + 5) * 8)            # the last row has no padding: flush against the guard
    assert a.used() == 3 * 5 * 8
    assert np.isnan(t.numpy()).all()
    t.copy_(torch.arange(15.0, dtype=torch.float64).view(3, 5))
    assert a.check() == []
    a.buf[start + 5 * 8] = 0                                                # the first padding byte of row 0
    a.buf[start + (7 + 6) * 8 + 3] = 0                                      # inside the second padding column of row 1
    a.buf[start + (2 * 7 + 5) * 8] = 0                                      # just after the last element
    assert a.check() == [("strided", "padding", 40), ("strided", "padding", 107), ("strided", "after", 1)]
    with pytest.raises(ValueError):
        a.take((3, 5), torch.float64, ld=4)


def test_default_owner_is_the_callers_file_and_line():
    a = arena()
    t = a.take(4, torch.uint8)
    line = test_default_owner_is_the_callers_file_and_line.__code__.co_firstlineno + 2
    a.buf[t.data_ptr() - a.buf.data_ptr() + 4] = 0
    assert a.check() == [("test_guarded_memory_cpu.py:%d" % line, "after", 1)]


def test_guarded_allocators_take_every_size_spelling(monkeypatch):
    a = arena(1 << 18)
    real = (torch.empty, torch.zeros, torch.empty_like, torch.tensor, torch.Tensor.to)
    with gm.guarded(monkeypatch, a):
        assert torch.empty is not real[0]
        got = [torch.empty(2, 3, dtype=torch.float64, device="cpu"), torch.empty((2, 3), dtype=torch.float64, device="cpu"),
               torch.empty(torch.Size([2, 3]), dtype=torch.float64, device="cpu"), torch.empty([2, 3], dtype=torch.float64),
               torch.empty(6, dtype=torch.float64, device=torch.device("cpu")).view(2, 3), torch.empty(size=(2, 3), dtype=torch.float64)]
        for t in got:
            assert tuple(t.shape) == (2, 3) and t.dtype == torch.float64 and np.isnan(t.numpy()).all()   # poison, from the arena
        z = [torch.zeros(5, dtype=torch.int32, device="cpu"), torch.zeros((5,), dtype=torch.int32), torch.zeros(torch.Size([5]), dtype=torch.int32)]
        for t in z:
            assert t.dtype == torch.int32 and t.tolist() == [0] * 5
        assert torch.zeros(3).dtype == torch.float32 and torch.zeros(3).tolist() == [0.0] * 3
        like = torch.empty_like(z[0])
        assert like.shape == z[0].shape and like.dtype == torch.int32 and like.tolist() == [-1] * 5
        assert torch.empty_like(z[0], dtype=torch.uint8).tolist() == [255] * 5
        assert torch.zeros_like(got[0]).tolist() == [[0.0] * 3] * 2
        assert torch.empty(0, dtype=torch.float64, device="cpu").numel() == 0
        lo, hi = a.buf.data_ptr(), a.buf.data_ptr() + a.nbytes
        for t in got + z + [like]:
            assert lo <= t.data_ptr() < hi and t.data_ptr() % 256 == 0
        n = a.count()
        # the other forms the package allocates with
        v = torch.tensor([1, 2, 3], dtype=torch.int32, device="cpu")
        c = torch.cat([v, v])
        s = torch.stack([v, v])
        k = v.clone()
        f = v.to(torch.float64)
        nc = s.t().contiguous()
        assert v.tolist() == [1, 2, 3] and c.tolist() == [1, 2, 3, 1, 2, 3] and s.tolist() == [[1, 2, 3]] * 2 and k.tolist() == [1, 2, 3]
        assert f.tolist() == [1.0, 2.0, 3.0] and nc.tolist() == [[1, 1], [2, 2], [3, 3]]
        for t in (v, c, s, k, f, nc):
            assert lo <= t.data_ptr() < hi
        assert a.count() == n + 6
        assert v.to(torch.int32) is v and v.contiguous() is v and a.count() == n + 6   # no copy, no allocation
        assert a.log["empty"] >= 7 and a.log["zeros"] >= 5 and a.log["cat"] == 1 and a.log["to"] == 1
        assert a.check() == []
    assert (torch.empty, torch.zeros, torch.empty_like, torch.tensor, torch.Tensor.to) == real
    assert "contiguous" not in torch.Tensor.__dict__ or torch.Tensor.contiguous is gm._REAL["contiguous"]
    t = torch.empty(3, dtype=torch.float64)
    assert not a.buf.data_ptr() <= t.data_ptr() < a.buf.data_ptr() + a.nbytes


def test_other_devices_and_pinned_requests_pass_through(monkeypatch):
    """an arena that stands for another device (its device is changed after it is built: there is no GPU here)"""
    a = arena()
    a.device = torch.device("meta")
    with gm.guarded(monkeypatch, a):
        t = torch.empty(4, dtype=torch.float64, device="cpu")
        z = torch.zeros((2, 2), dtype=torch.uint8)
        e = torch.empty_like(z)
        m = torch.empty(7, dtype=torch.float32, device="meta")     # the arena's device: from the arena
        assert m.shape == (7,) and a.count() == 1
        for x in (t, z, e, torch.tensor([1.0]), torch.cat([z, z]), z.clone(), z.to(torch.float64)):
            assert not a.buf.data_ptr() <= x.data_ptr() < a.buf.data_ptr() + a.nbytes
        assert z.tolist() == [[0, 0], [0, 0]] and a.count() == 1
    a.device = torch.device("cpu")
    seen = []
    monkeypatch.setitem(gm._REAL, "empty", lambda *args, **kw: seen.append(kw) or torch.Tensor())
    with gm.guarded(monkeypatch, a):
        torch.empty(4, dtype=torch.uint8, pin_memory=True)         # pinned: the real function gets it, whatever the device
        assert seen == [{"dtype": torch.uint8, "pin_memory": True}] and a.count() == 1


def toy_kernel(n):
    """reads its torch.empty output before writing it: out[k] += k"""
    out = torch.empty(n, dtype=torch.int32, device="cpu")
    out += torch.arange(n, dtype=torch.int32)
    return out


def toy_kernel_zeroed(n):
    out = torch.zeros(n, dtype=torch.int32, device="cpu")
    out += torch.arange(n, dtype=torch.int32)
    return out


def test_a_read_before_write_differs_between_the_patterns(monkeypatch):
    a = arena()
    got, good = [], []
    for pattern in ("ff", ("random", 1)):
        a.reset(pattern)
        with gm.guarded(monkeypatch, a):
            got.append(toy_kernel(9).numpy().tobytes())
            good.append(toy_kernel_zeroed(9).numpy().tobytes())
        assert a.check() == []
    assert got[0] != got[1] and good[0] == good[1] == np.arange(9, dtype=np.int32).tobytes()


def test_functions_are_restored_after_an_exception(monkeypatch):
    real = torch.empty
    with pytest.raises(ZeroDivisionError):
        with gm.guarded(monkeypatch, arena()):
            1 / 0
    assert torch.empty is real and torch.Tensor.to is gm._REAL["to"]
