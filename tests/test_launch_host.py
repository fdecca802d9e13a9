"""fieldconv_amd._launch on the host: the NULL rule of `ptr`, the zero-byte rule of `scratch` under each floor, and the one integer
check `whole` under both acceptance rules."""
import numpy as np
import pytest
import torch

from fieldconv_amd import _launch


def test_ptr_is_null_for_none_and_for_an_empty_tensor():
    assert _launch.ptr(None) is None
    assert _launch.ptr(torch.empty(0)) is None
    assert _launch.ptr(torch.ones(4)[4:]) is None          # empty, though its storage is live
    t = torch.ones(1)
    assert _launch.ptr(t).value == t.data_ptr() != 0


@pytest.mark.parametrize('floor,zero_bytes', [(0, 0), (1, 1), (None, None)])
def test_scratch_zero_byte_rule(floor, zero_bytes):
    cpu = torch.device('cpu')
    ws = _launch.scratch(0, cpu, floor)
    if zero_bytes is None:
        assert ws is None
    else:
        assert ws.dtype == torch.uint8 and ws.device == cpu and tuple(ws.shape) == (zero_bytes,)
    ws = _launch.scratch(5, cpu, floor)
    assert ws.dtype == torch.uint8 and ws.device == cpu and tuple(ws.shape) == (5,)


@pytest.mark.parametrize('integral_floats', [False, True])
def test_whole(integral_floats):
    def whole(v, lo=0, hi=8, where=''):
        return _launch.whole(v, lo, hi, 'op', 'k', where, integral_floats)
    for v in (3, np.int64(3), torch.tensor(3)):
        n = whole(v)
        assert n == 3 and type(n) is int
    if integral_floats:
        n = whole(3.0)
        assert n == 3 and type(n) is int
    else:
        with pytest.raises(ValueError, match=r'op: k must be an integer in \[0, 8\], got 3\.0'):
            whole(3.0)
    for bad in (1.5, True, '3', None, 9, -1, float('nan'), float('inf')):
        with pytest.raises(ValueError, match=r'op: k must be an integer in \[0, 8\], got '):
            whole(bad)
    assert whole(0) == 0 and whole(8) == 8
    with pytest.raises(ValueError, match=r"op: k of mesh 2 must be an integer in \[1, 4\], got '3'"):
        whole('3', 1, 4, ' of mesh 2')
