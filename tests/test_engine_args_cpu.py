"""
jubjub_amd.engine._Arg (no GPU): a host argument reaches the library as the bytes it holds, never through a cast of its values.  An array of
another dtype is a TypeError, as it is for a torch tensor; bytes-like objects and sequences of byte values are accepted.
"""
import numpy as np
import pytest

from jubjub_amd.engine import _Arg


def test_uint8_arrays_pass_unchanged():
    a = np.arange(64, dtype=np.uint8).reshape(2, 32)
    arg = _Arg(a, 32)
    assert arg.n == 2 and arg.keep is a and arg.ptr == a.ctypes.data and not arg.torch
    b = np.arange(128, dtype=np.uint8).reshape(2, 64)[:, ::2]                         # not contiguous: copied, same values
    arg = _Arg(b, 32)
    assert arg.n == 2 and arg.keep.flags.c_contiguous and (arg.keep == b).all()
    assert _Arg(np.zeros((0, 32), np.uint8), 32).n == 0 and _Arg(np.zeros((0, 32), np.uint8), 32).ptr is None


@pytest.mark.parametrize("dtype", [np.int8, np.int16, np.int32, np.int64, np.uint16, np.uint32, np.uint64, np.float32, np.float64, np.bool_])
def test_other_dtypes_are_a_type_error(dtype):
    with pytest.raises(TypeError):
        _Arg(np.zeros((1, 32), dtype), 32)


def test_the_three_silent_casts_are_gone():
    with pytest.raises(TypeError):
        _Arg(np.arange(250, 282, dtype=np.int64), 32)                                 # wrapped to 250 ... 255, 0, 1, ...
    with pytest.raises(TypeError):
        _Arg(np.ones((8, 4), np.uint64), 32)                                          # limbs: read as one garbage scalar
    with pytest.raises(TypeError):
        _Arg(np.full(32, 1.5), 32)                                                    # truncated


def test_bytes_like_objects_and_byte_lists():
    raw = bytes(range(32))
    for x in (raw, bytearray(raw), memoryview(raw)):
        arg = _Arg(x, 32)
        assert arg.n == 1 and bytes(arg.keep) == raw
    assert bytes(_Arg(memoryview(np.arange(32, dtype=np.int8)), 32).keep) == raw     # one-byte items are bytes
    for view in (memoryview(np.zeros(4, np.int64)), memoryview(np.zeros(64, np.uint8))[::2]):
        with pytest.raises(TypeError):
            _Arg(view, 32)                                                            # wider items, a strided view
    arg = _Arg(list(range(224, 256)), 32)
    assert arg.n == 1 and arg.keep.dtype == np.uint8 and list(arg.keep) == list(range(224, 256))
    assert _Arg([], 32).n == 0
    for bad in ([256] + [0] * 31, [-1] + [0] * 31):
        with pytest.raises(ValueError):
            _Arg(bad, 32)
    with pytest.raises(TypeError):
        _Arg([0.5] * 32, 32)
    with pytest.raises(ValueError):
        _Arg(bytes(33), 32)                                                           # the length check still holds


def test_torch_tensors_of_another_dtype_are_a_type_error():
    torch = pytest.importorskip("torch")
    with pytest.raises(TypeError):
        _Arg(torch.zeros((1, 32), dtype=torch.int64), 32)
    assert _Arg(torch.zeros((3, 32), dtype=torch.uint8), 32).n == 3
