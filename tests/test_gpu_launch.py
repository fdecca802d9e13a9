"""fieldconv_amd._launch on the device: the fast stream lookup names the stream torch calls current, and the device guard is the
shared no-op exactly when the device already is the current one."""
import pytest
import torch

from fieldconv_amd import _launch

pytestmark = pytest.mark.gpu


def test_stream_and_device_guard():
    def raw():
        return _launch.stream().value or 0          # (a NULL c_void_p reads back as None: the default stream)
    assert raw() == torch.cuda.current_stream().cuda_stream
    with torch.cuda.stream(torch.cuda.Stream()):
        assert torch.cuda.current_stream() != torch.cuda.default_stream()
        assert raw() == torch.cuda.current_stream().cuda_stream != 0
    current = torch.cuda.current_device()
    assert _launch.on(torch.device('cuda', current)) is _launch.NO_GUARD
    with _launch.NO_GUARD:
        assert torch.cuda.current_device() == current
    guard = _launch.on(torch.device('cuda'))          # no index: the real guard, which resolves to the current device
    assert guard is not _launch.NO_GUARD
    with guard:
        assert torch.cuda.current_device() == current
        assert torch.empty(1, device='cuda').device.index == current
    assert torch.cuda.current_device() == current
