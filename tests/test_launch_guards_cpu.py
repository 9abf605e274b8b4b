"""The two launch instruments of tests/helpers.py, guarded_calls() and poisoned_empties(), on the CPU: no GPU and no library.  A fake
object stands in for the loaded library; its entry points are Python callables that write through ctypes into CPU tensors, handed the
addresses _hip.call would hand a kernel.  Every call passes stream=0, so torch's current stream is never asked for."""
import ctypes
import types

import pytest
import torch

from meta_interpolation_amd import _hip
from tests.helpers import CANARY, GUARD_PAD, guarded_calls, poisoned_empties


def _floats(addr, n):
    return (ctypes.c_float * n).from_address(addr)


def _fill(dst, n, start, value, stream):
    """dst[start : start + n] = value + index (start may be negative or reach past the end: that is the caller's bug under test)"""
    a = _floats(dst + 4 * start, n)
    for i in range(n):
        a[i] = value + i
    return 0


def _axpy(x, y, ws, n, ws_at, stream):
    """y = 2 * x through the workspace; ws_at: the workspace float the kernel uses for its (one) intermediate"""
    xs, ys, w = _floats(x, n), _floats(y, n), _floats(ws + 4 * ws_at, 1)
    for i in range(n):
        w[0] = 2 * xs[i]
        ys[i] = w[0]
    return 0


def _fill_many(n, ptrs, raw, count, stream):
    """every pointer of the host array `ptrs`, and the raw address `raw`, gets `count` floats 1, 2, ..."""
    for p in list(ptrs[:n]) + [raw]:
        a = _floats(p, count)
        for i in range(count):
            a[i] = i + 1.0
    return 0


def _fails(stream):
    return -2


@pytest.fixture
def fake_lib(monkeypatch):
    monkeypatch.setattr(_hip, "_lib", types.SimpleNamespace(fill=_fill, axpy=_axpy, fill_many=_fill_many, fails=_fails))


def _guarded():
    return guarded_calls(device="cpu")


def test_a_write_past_the_end_of_the_output_is_named(fake_lib):
    out = torch.zeros(5)
    with _guarded() as rec, pytest.raises(AssertionError) as exc:
        _hip.call("t", "fill", out, 6, 0, 1.0, stream=0)                     # six floats into five
    msg = str(exc.value)
    assert "fill" in msg and "argument 0" in msg and "after" in msg and "byte offset 20" in msg, msg
    assert rec.guarded == {"fill": 1}
    assert out.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]                          # the in-bounds part came back all the same


def test_a_write_before_the_start_of_the_output_is_named(fake_lib):
    out = torch.zeros(5)
    with _guarded(), pytest.raises(AssertionError) as exc:
        _hip.call("t", "fill", out, 2, -1, 1.0, stream=0)
    msg = str(exc.value)
    assert "fill" in msg and "argument 0" in msg and "before" in msg and "byte offset -4" in msg, msg


def test_a_write_past_the_end_of_a_workspace_argument_is_named(fake_lib):
    x, y, ws = torch.arange(4.0), torch.zeros(4), torch.zeros(3)
    with _guarded(), pytest.raises(AssertionError) as exc:
        _hip.call("t", "axpy", x, y, ws, 4, 3, stream=0)                      # the workspace has floats 0..2
    msg = str(exc.value)
    assert "axpy" in msg and "argument 2" in msg and "after" in msg and "byte offset 12" in msg, msg
    with _guarded() as rec:
        _hip.call("t", "axpy", x, y, ws, 4, 2, stream=0)
    assert y.tolist() == [0.0, 2.0, 4.0, 6.0] and ws.tolist() == [0.0, 0.0, 6.0] and rec.guarded == {"axpy": 1}


def test_a_write_into_the_last_canary_float_is_caught(fake_lib):
    out = torch.zeros(3)
    with _guarded(), pytest.raises(AssertionError) as exc:
        _hip.call("t", "fill", out, 1, 3 + GUARD_PAD - 1, 1.0, stream=0)      # the last canary float
    assert "byte offset %d" % (4 * (3 + GUARD_PAD - 1)) in str(exc.value)


def test_in_bounds_through_a_view_with_a_storage_offset(fake_lib):
    buf = torch.full((10,), -1.0)
    view = buf[3:7]
    assert view.storage_offset() == 3
    with _guarded():
        _hip.call("t", "fill", view, 4, 0, 10.0, stream=0)
    assert buf.tolist() == [-1.0] * 3 + [10.0, 11.0, 12.0, 13.0] + [-1.0] * 3


def test_in_bounds_through_two_views_of_one_storage(fake_lib):
    buf = torch.zeros(8)
    buf[:4] = torch.arange(4.0)
    ws = torch.zeros(1)
    with _guarded() as rec:
        _hip.call("t", "axpy", buf[:4], buf[4:], ws, 4, 0, stream=0)          # reads one half, writes the other: one copy serves both
    assert buf.tolist() == [0.0, 1.0, 2.0, 3.0, 0.0, 2.0, 4.0, 6.0] and rec.guarded == {"axpy": 1}
    x = torch.arange(4.0)
    with _guarded():
        _hip.call("t", "axpy", x, x, ws, 4, 0, stream=0)                      # in place
    assert x.tolist() == [0.0, 2.0, 4.0, 6.0]


def test_in_bounds_through_a_raw_pointer_sum_and_a_pointer_array(fake_lib):
    buf, other = torch.zeros(12), torch.zeros(2)
    # buf is a tensor argument (so it is substituted); the host array points at its floats 2 and 6, the raw sum at float 10; `other`
    # is reached through the array alone and stays where it is
    arr = _hip.ptr_array([buf[2:], buf[6:], other])
    with _guarded():
        _hip.call("t", "fill", buf, 1, 0, 9.0, stream=0)
        _hip.call("t", "fill_many", 3, arr, buf.data_ptr() + 40, 2, stream=0)
        # fill_many takes no tensor: nothing is substituted, everything is written in place
    assert buf.tolist() == [9.0, 0.0, 1.0, 2.0, 0.0, 0.0, 1.0, 2.0, 0.0, 0.0, 1.0, 2.0] and other.tolist() == [1.0, 2.0]
    buf.zero_(), other.zero_()
    before = [arr[i] for i in range(3)]

    def fill_many_of(anchor, n, ptrs, raw, count, stream):
        return _fill_many(n, ptrs, raw, count, stream)
    _hip._lib.fill_many_of = fill_many_of
    with _guarded():
        _hip.call("t", "fill_many_of", buf, 3, arr, buf.data_ptr() + 40, 2, stream=0)
    assert buf.tolist() == [0.0, 0.0, 1.0, 2.0, 0.0, 0.0, 1.0, 2.0, 0.0, 0.0, 1.0, 2.0] and other.tolist() == [1.0, 2.0]
    assert [arr[i] for i in range(3)] == before                               # the caller's array is not rewritten
    with _guarded(), pytest.raises(AssertionError) as exc:
        _hip.call("t", "fill_many_of", buf, 3, arr, buf.data_ptr() + 44, 2, stream=0)     # the raw sum's second float is past the end
    assert "fill_many_of" in str(exc.value) and "argument 0" in str(exc.value) and "after" in str(exc.value)


def test_a_write_into_the_neighbouring_slice_of_the_same_storage_is_not_reported(fake_lib):
    """The limit of a guard per storage (guarded_calls' docstring states it): the slice tests of the ops cover this."""
    buf = torch.zeros(8)
    with _guarded():
        _hip.call("t", "fill", buf[:4], 5, 0, 1.0, stream=0)
    assert buf.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0, 0.0, 0.0, 0.0]


def test_the_call_comes_back_after_an_exception_and_errors_pass_through(fake_lib):
    call = _hip.call
    with pytest.raises(AssertionError):
        with _guarded():
            assert _hip.call is not call
            _hip.call("t", "fill", torch.zeros(2), 3, 0, 1.0, stream=0)
    assert _hip.call is call
    with pytest.raises(_hip.SavfiHipError, match="fails: SAVFI_E_SHAPE"):
        with _guarded():
            _hip.call("t", "fails", stream=0)
    assert _hip.call is call
    with pytest.raises(KeyError):
        with _guarded():
            raise KeyError("x")
    assert _hip.call is call


def test_launches_still_go_through_launch_and_check_by_name(fake_lib, monkeypatch):
    seen = []
    monkeypatch.setattr(_hip, "launch", lambda name, fn, nbytes=0, flops=0: (seen.append((name, nbytes, flops)), fn())[1])
    out = torch.zeros(2)
    with _guarded():
        _hip.call("timer", "fill", out, 2, 0, 1.0, nbytes=8, flops=3, stream=0)
    assert seen == [("timer", 8, 3)] and out.tolist() == [1.0, 2.0]


DTYPES = [torch.float32, torch.float64, torch.uint8, torch.int64]


def _poisoned(t):
    if t.dtype.is_floating_point:
        return bool(torch.isnan(t).all())
    return bool((t == torch.iinfo(t.dtype).max).all())


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_every_allocation_form_comes_back_filled(dtype):
    like = torch.zeros(3, 5, dtype=dtype)
    with poisoned_empties() as rec:
        made = [torch.empty(3, 5, dtype=dtype), torch.empty((2, 7), dtype=dtype, device="cpu"), torch.empty_like(like),
                like.new_empty((4, 2)), like.new_empty(6)]
        zeros = torch.zeros(3, 5, dtype=dtype)
    assert all(t.dtype == dtype and _poisoned(t) for t in made)
    assert [tuple(t.shape) for t in made] == [(3, 5), (2, 7), (3, 5), (4, 2), (6,)]
    assert rec.filled == 5
    assert bool((zeros == 0).all())


def test_bool_and_empty_tensors_are_left_alone_and_leaves_can_be_filled():
    with poisoned_empties() as rec:
        b = torch.empty(4, dtype=torch.bool)
        e = torch.empty(0)
        leaf = torch.empty(3, requires_grad=True)
    assert b.dtype == torch.bool and e.numel() == 0 and rec.filled == 1
    assert leaf.requires_grad and leaf.is_leaf and bool(torch.isnan(leaf).all())


def test_the_originals_come_back_also_after_an_exception():
    originals = (torch.empty, torch.empty_like, torch.Tensor.new_empty)
    with poisoned_empties():
        assert torch.empty is not originals[0] and torch.empty_like is not originals[1] and torch.Tensor.new_empty is not originals[2]
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == originals
    with pytest.raises(KeyError):
        with poisoned_empties():
            raise KeyError("x")
    assert (torch.empty, torch.empty_like, torch.Tensor.new_empty) == originals


def test_the_canary_is_the_suites():
    assert CANARY == 7777.0 and GUARD_PAD % 128 == 0          # 128 floats = 512 bytes: the pad keeps every pointer's alignment
