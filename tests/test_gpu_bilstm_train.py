"""The BiLSTM training entry points of the C ABI, called directly -- amtx_bilstm_h_pack_device, amtx_bilstm_h_train_fwd,
amtx_bilstm_h_train_bwd (csrc/lstm.hip, two planes) -- against the float64 recurrence of tests/lstm_ref.py, at every built hidden size:
128 (register-stationary pair) and 256 / 384 / 512 (bilstm_stream_kernel / bilstm_stream_bwd_kernel, one instantiation each).

Cases (B, T, groups, xproj scale) and what each reaches:
    (1, 1, 1, 1)   three idle clip slots, no recurrence, the `s + 1 < T` clamp of both prefetches
    (1, 2, 1, 1)   the shortest recurrence
    (3, 5, 2, 1)   two LSTMs in one launch: the group strides of xproj, fragments, save and dxproj
    (4, 19, 1, 1)  a full backward block
    (5, 19, 2, 1)  a backward block that holds one clip
    (17, 7, 1, 1)  the streaming forward's second 16-clip block, one clip in it
    (3, 96, 1, 1)  ring phase and the dc chain over many steps
    (5, 19, 1, 6)  saturated gates
Tolerances and their derivation: tests/lstm_ref.py (TOL_OUT, TOL_SAVE, TOL_DX); tests/test_lstm_ref.py shows what they can see."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')

pytestmark = pytest.mark.gpu

from amt_tools_amd import _lib            # noqa: E402
from poison import fill_storage           # noqa: E402
import lstm_ref as R                      # noqa: E402

F32 = 1
DEV = 'cuda:0'
NAN_BITS = -1                             # 0xFFFFFFFF: a NaN as fp32


def _poisoned(clips, *shape):
    """fp32 [clips + 1][*shape] on the device, every byte 0xFF (NaN): the kernels get the first `clips`, the last one must stay as it is."""
    return fill_storage(torch.empty((clips + 1,) + shape, dtype=torch.float32, device=DEV), 0xFF)


def _bits(t):
    return t.view(torch.int32)


def _check_bounds(buf, clips, what):
    torch.cuda.synchronize()              # a fault of the launch before surfaces here: nothing more is launched after it
    assert not torch.isnan(buf[:clips]).any().item(), f'{what}: NaN left inside the valid region'
    assert bool((_bits(buf[clips:]) == NAN_BITS).all().item()), f'{what}: written past the last clip'


def _host_fragments(whh_f, whh_b, H):
    out = np.zeros(int(_lib.call('amtx_bilstm_h_packed_elems', H, 2)), dtype=np.uint16)
    _lib.call('amtx_bilstm_h_pack', np.ascontiguousarray(whh_f.numpy()), np.ascontiguousarray(whh_b.numpy()), H, 2, out)
    return out


def _forward(xproj_d, frag_fwd, H, B, T, G):
    out, save = _poisoned(G * B, T, 2 * H), _poisoned(G * B, T, 2, 5, H)
    _lib.call('amtx_bilstm_h_train_fwd', xproj_d, frag_fwd, H, 2, out, save, B, T, G, device=DEV)
    _check_bounds(out, G * B, 'out')
    _check_bounds(save, G * B, 'save')
    return out, save


def _backward(dout_d, save, frag_bwd, H, B, T, G):
    dx = _poisoned(G * B, T, 2, 4 * H)
    _lib.call('amtx_bilstm_h_train_bwd', dout_d, save, frag_bwd, H, 2, dx, B, T, G, device=DEV)
    _check_bounds(dx, G * B, 'dxproj')
    return dx


@pytest.mark.parametrize('B,T,G,scale', R.CASES)
@pytest.mark.parametrize('H', R.HIDDEN)
def test_bilstm_train_kernels_match_the_float64_recurrence(H, B, T, G, scale):
    ref = R.reference(H, B, T, G, scale)                     # shared, read-only
    xproj_d, dout_d = ref['xproj'].to(DEV), ref['dout'].to(DEV)
    n = int(_lib.call('amtx_bilstm_h_packed_elems', H, 2))
    assert n == 2 * 4 * H * H * 2

    # ---- packing: the device packer's forward fragments are the host packer's
    whh_f_d, whh_b_d = ref['whh_f'].to(DEV), ref['whh_b'].to(DEV)
    frag_fwd = fill_storage(torch.empty((G, n), dtype=torch.int16, device=DEV), 0xFF)
    frag_bwd = fill_storage(torch.empty((G, n), dtype=torch.int16, device=DEV), 0xFF)
    for g in range(G):
        _lib.call('amtx_bilstm_h_pack_device', whh_f_d[g], whh_b_d[g], H, 2, frag_fwd[g], frag_bwd[g], device=DEV)
    torch.cuda.synchronize()
    host = [_host_fragments(ref['whh_f'][g], ref['whh_b'][g], H) for g in range(G)]
    for g in range(G):
        assert frag_fwd[g].cpu().numpy().view(np.uint16).tobytes() == host[g].tobytes(), f'forward fragments of group {g}'

    # ---- forward
    out, save = _forward(xproj_d, frag_fwd, H, B, T, G)
    out_v, save_v = out[:G * B].reshape(G, B, T, 2 * H), save[:G * B].reshape(G, B, T, 2, 5, H)
    err_out = (out_v.cpu().double() - ref['out']).abs().max().item()
    save_scale = max(1.0, ref['save'][..., 4, :].abs().max().item())
    err_save = [(save_v[..., k, :].cpu().double() - ref['save'][..., k, :]).abs().max().item() / save_scale for k in range(5)]

    # ---- the training forward is the inference forward (one instantiation, `save` a runtime argument): same bits on the host's fragments
    for g in range(G):
        inf = _poisoned(B, T, 2 * H)
        _lib.call('amtx_bilstm_h_fwd', xproj_d[g], torch.from_numpy(host[g].view(np.int16)).to(DEV), H, 2, F32, inf, B, T, device=DEV)
        _check_bounds(inf, B, 'inference out')
        assert torch.equal(_bits(inf[:B]), _bits(out_v[g])), f'training and inference forward differ (group {g})'

    # ---- backward: on the kernel's own save (the production chain), and alone on the reference's save rounded to fp32
    dx_scale = ref['dxproj'].abs().max().item()
    dx = _backward(dout_d, save, frag_bwd, H, B, T, G)
    err_dx = (dx[:G * B].reshape(G, B, T, 2, 4 * H).cpu().double() - ref['dxproj']).abs().max().item() / dx_scale
    save_ref = _poisoned(G * B, T, 2, 5, H)
    save_ref[:G * B] = ref['save'].float().reshape(G * B, T, 2, 5, H).to(DEV)
    dx_alone = _backward(dout_d, save_ref, frag_bwd, H, B, T, G)
    err_dx_alone = (dx_alone[:G * B].reshape(G, B, T, 2, 4 * H).cpu().double() - ref['dxproj']).abs().max().item() / dx_scale

    # ---- determinism: no atomics in either recurrence
    out2, save2 = _forward(xproj_d, frag_fwd, H, B, T, G)
    dx2 = _backward(dout_d, save, frag_bwd, H, B, T, G)
    same = [torch.equal(_bits(a), _bits(b)) for a, b in ((out, out2), (save, save2), (dx, dx2))]

    print(f'LSTMERR H={H} case=({B},{T},{G},{scale}) out={err_out:.3e} save=' + '/'.join(f'{e:.3e}' for e in err_save) +
          f' save_scale={save_scale:.3g} dx={err_dx:.3e} dx_alone={err_dx_alone:.3e}')
    assert err_out < R.TOL_OUT, err_out
    for k, name in enumerate('ifgoc'):
        assert err_save[k] < R.TOL_SAVE, (name, err_save[k])
    assert err_dx < R.TOL_DX, err_dx
    assert err_dx_alone < R.TOL_DX, err_dx_alone
    assert same == [True, True, True], same
