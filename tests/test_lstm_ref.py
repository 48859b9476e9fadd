"""tests/lstm_ref.py without any kernel: the float64 recurrences agree with torch.nn.LSTM in float64, and the tolerances the GPU tests
hold the kernels to (tests/test_gpu_bilstm_train.py) are small enough to see one lost bf16 plane or one lost k-step of either mat-vec."""
import pytest

torch = pytest.importorskip('torch')

import lstm_ref as R            # noqa: E402


@pytest.mark.parametrize('B,T', [(1, 1), (3, 5), (5, 19)])
@pytest.mark.parametrize('H', [128, 256])
def test_reference_matches_torch_lstm_in_float64(H, B, T):
    """nn.LSTM over the input [xproj of direction 0 | xproj of direction 1] with W_ih of each direction selecting its half (ones and
    zeros: exact products) and zero biases computes the recurrence on xproj itself; its autograd gives d(out . dout) / d(xproj)."""
    case = R.make_case(H, B, T)
    whh_f, whh_b = case['whh_f'][0].double(), case['whh_b'][0].double()
    lstm = torch.nn.LSTM(8 * H, H, batch_first=True, bidirectional=True).double()
    eye, zero = torch.eye(4 * H, dtype=torch.float64), torch.zeros(4 * H, 4 * H, dtype=torch.float64)
    with torch.no_grad():
        lstm.weight_ih_l0.copy_(torch.cat([eye, zero], dim=1))
        lstm.weight_ih_l0_reverse.copy_(torch.cat([zero, eye], dim=1))
        lstm.weight_hh_l0.copy_(whh_f)
        lstm.weight_hh_l0_reverse.copy_(whh_b)
        for name in ('bias_ih_l0', 'bias_hh_l0', 'bias_ih_l0_reverse', 'bias_hh_l0_reverse'):
            getattr(lstm, name).zero_()
    x = case['xproj'][0].double().reshape(B, T, 8 * H).requires_grad_(True)
    dout = case['dout'][0].double()
    y = lstm(x)[0]
    (y * dout).sum().backward()

    out, save = R.forward(case['xproj'][0], case['whh_f'][0], case['whh_b'][0])
    dx = R.backward(save, case['whh_f'][0], case['whh_b'][0], case['dout'][0])
    assert out.dtype == save.dtype == dx.dtype == torch.float64
    assert (out - y.detach()).abs().max().item() <= 1e-12
    assert (dx.reshape(B, T, 8 * H) - x.grad).abs().max().item() <= 1e-12
    # save is in the kernels' layout: h = o tanh(c) from its own components, gates inside their ranges
    h = save[:, :, :, 3] * torch.tanh(save[:, :, :, 4])
    assert torch.equal(h.reshape(B, T, 2 * H), out)
    assert save[:, :, :, (0, 1, 3)].min() > 0 and save[:, :, :, (0, 1, 3)].max() < 1 and save[:, :, :, 2].abs().max() < 1


def test_tolerances_are_under_their_caps():
    assert 0 < R.TOL_OUT <= R.CAP_OUT == 3e-5
    assert 0 < R.TOL_SAVE <= R.CAP_SAVE == 3e-5
    assert 0 < R.TOL_DX <= R.CAP_DX == 3.2e-5


def test_cases_are_the_eight_of_the_gpu_suite():
    assert R.HIDDEN == (128, 256, 384, 512)
    assert R.CASES == ((1, 1, 1, 1), (1, 2, 1, 1), (3, 5, 2, 1), (4, 19, 1, 1), (5, 19, 2, 1), (17, 7, 1, 1), (3, 96, 1, 1), (5, 19, 1, 6))
    a, b = R.make_case(128, 3, 5, 2), R.make_case(128, 3, 5, 2)
    assert all(torch.equal(a[k], b[k]) for k in a)                       # seeded
    assert a['whh_f'].abs().max() <= 0.15 and R.make_case(256, 1, 1)['whh_b'].abs().max() <= 0.1
    assert not torch.equal(a['xproj'][0], a['xproj'][1])


def _ksteps(n):
    return sorted({0, n // 2, n - 1})                                     # start, middle and end of the k range


@pytest.mark.parametrize('B,T', [(5, 19), (3, 96)])
@pytest.mark.parametrize('H', [128, 512])
def test_tolerances_have_teeth(H, B, T):
    """Every single-operand bf16 rounding of a mat-vec moves the reference by at least 10 x the tolerance of what that mat-vec feeds,
    every dropped 32-wide k-step by at least 100 x: a kernel with that defect cannot pass tests/test_gpu_bilstm_train.py."""
    ref = R.reference(H, B, T)
    xproj, whh_f, whh_b, dout = ref['xproj'][0], ref['whh_f'][0], ref['whh_b'][0], ref['dout'][0]
    out, save, dx = ref['out'][0], ref['save'][0], ref['dxproj'][0]
    save_scale = max(1.0, save[:, :, :, 4].abs().max().item())
    dx_scale = dx.abs().max().item()

    for mutate, factor in [(('bf16', 'w'), 10), (('bf16', 'v'), 10)] + [(('drop', ks), 100) for ks in _ksteps(H // 32)]:
        m_out, m_save = R.forward(xproj, whh_f, whh_b, mutate=mutate)
        d_out = (m_out - out).abs().max().item()
        d_save = (m_save - save).abs().max().item()
        print(f'H {H} ({B},{T}) forward {mutate}: out {d_out:.3g} (x{d_out / R.TOL_OUT:.0f}), save {d_save:.3g} (x{d_save / (R.TOL_SAVE * save_scale):.0f})')
        assert d_out >= factor * R.TOL_OUT, (mutate, d_out)
        assert d_save >= factor * R.TOL_SAVE * save_scale, (mutate, d_save)

    for mutate, factor in [(('bf16', 'w'), 10), (('bf16', 'v'), 10)] + [(('drop', ks), 100) for ks in _ksteps(4 * H // 32)]:
        m_dx = R.backward(save, whh_f, whh_b, dout, mutate=mutate)
        d_dx = (m_dx - dx).abs().max().item() / dx_scale
        print(f'H {H} ({B},{T}) backward {mutate}: dxproj {d_dx:.3g} of max (x{d_dx / R.TOL_DX:.0f})')
        assert d_dx >= factor * R.TOL_DX, (mutate, d_dx)

