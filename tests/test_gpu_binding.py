"""GPU check of the binding's call helper: _lib.call(..., device=dev) launches what the spelled-out form launches -- same device, same
(non-default) current stream, same arguments -- and refuses a wrong argument count before anything reaches the device."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
pytestmark = pytest.mark.gpu

from amt_tools_amd import _lib          # noqa: E402


def test_call_fills_device_and_stream_like_the_spelled_out_form():
    B, N = 3, 5000
    dev = torch.device('cuda', 0)
    L = _lib.lib()
    host = torch.from_numpy(np.random.default_rng(11).standard_normal((B, N)).astype(np.float32) * np.array([[0.1], [1.0], [20.0]], dtype=np.float32))
    stream = torch.cuda.Stream(device=dev)
    assert stream.cuda_stream != torch.cuda.default_stream(dev).cuda_stream
    with torch.cuda.stream(stream):
        audio = host.to(dev, non_blocking=False) * 1.0                   # produced on `stream`: the launches below must queue behind it
        ws = _lib.alloc_workspace(int(_lib.call('amtx_rms_norm_workspace_bytes', B, N)), dev)
        old, new, untouched = torch.empty_like(audio), torch.empty_like(audio), torch.full_like(audio, -7.0)
        with torch.cuda.device(dev):
            assert _lib.current_stream(dev).value == stream.cuda_stream
            _lib.check(L.amtx_rms_norm(_lib.ptr(audio), N, N, B, _lib.ptr(old), N, _lib.ptr(ws), ws.numel(), _lib.current_stream(dev)), 'amtx_rms_norm')
        assert _lib.call('amtx_rms_norm', audio, N, N, B, new, N, ws, ws.numel(), device=dev) == 0
        for args in ((audio, N, N, B, untouched, N, ws), (audio, N, N, B, untouched, N, ws, ws.numel(), None)):
            with pytest.raises(TypeError):                                # one argument short / the stream passed as well: nothing is enqueued
                _lib.call('amtx_rms_norm', *args, device=dev)
    stream.synchronize()
    assert torch.equal(old, new) and bool((untouched == -7.0).all())
    rms = new.double().pow(2).mean(dim=1).sqrt()
    assert float((rms - 1.0).abs().max()) < 1e-5
