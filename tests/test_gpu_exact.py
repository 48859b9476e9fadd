"""The matrix kernels, with NO tolerance: operands on an integer grid (tests/exact_inputs.py) for which a kernel whose arithmetic is only
multiply and add has one right answer, bit for bit, whatever its tiling, k-order or split contraction -- the float64 product.

EXACTNESS CONDITION (a precondition, asserted on the generated operands before anything is launched): every operand is exactly what the
kernel feeds the matrix cores (representable in bf16, or equal to hi + lo of the split-bf16 planes); every product of two such operands is
exact in fp32; and sum_k |a||w| + |bias|, divided by the grid step of the products and maximised over the outputs, is at most 2^21, so
every partial sum in any order is an fp32 number.  HEADROOM: fp32 holds 2^24 grid steps; the three spare bits are there because how the
bf16 matrix instructions accumulate internally had NOT been measured before this file existed -- that they keep every bit of an fp32
accumulator at these magnitudes is an assumption, and these tests are its first measurement.  (A failure that disappears when the
operand magnitudes are halved would be that assumption failing, not a kernel.)

A dropped, doubled or mispaired term moves some output by at least one grid step: every comparison here is torch.equal.  Kernels that write
bf16 or two planes are held to the exact value rounded once, round to nearest even; the operands make outputs that need that rounding,
ties among them.  One-sided fractional rule: only one operand of a product has a low plane, so the lo.lo term the split arithmetic drops is
zero and the reference is the true product.  tests/test_exact_inputs.py proves all of this for the references alone, on the CPU."""
import numpy as np
import pytest

torch = pytest.importorskip('torch')
import torch.nn.functional as F   # noqa: E402

pytestmark = pytest.mark.gpu

from amt_tools_amd import _lib   # noqa: E402
import exact_inputs as X         # noqa: E402
from exact_inputs import BF16, F32, SPLIT   # noqa: E402

NAN16 = 0x7fc0
GEMM_SWITCHES = ('AMTX_GEMM_NO_SKINNY', 'AMTX_GEMM_PP', 'AMTX_GEMM_NO_PP', 'AMTX_GEMM_NO_SPLIT_DMA')


def _route(*args):
    """exact_inputs.route, which answers for the default routing only: with an A/B switch of gemm.hip set the ids below would lie."""
    import os
    assert not [s for s in GEMM_SWITCHES if s in os.environ], 'the exact GEMM tests name the default routes: unset the AMTX_GEMM_* switches'
    return X.route(*args)


def _stream():
    return _lib.current_stream()


def _ids(cases):
    return [f'{r}-{m}x{n}x{k}' for r, m, n, k in cases]


def _pack_linear(w, planes):
    L = _lib.lib()
    n, k = w.shape
    packed = np.zeros(L.amtx_linear_packed_elems(n, k, planes), dtype=np.uint16)
    _lib.check(L.amtx_linear_pack(_lib.ptr(w.numpy()), n, k, planes, _lib.ptr(packed)))
    return torch.from_numpy(packed.view(np.int16)).cuda()


def _padded(a, dtype):
    """`a` on the device with lda = K + 8 and NaN in the pad columns, which no kernel may read."""
    m, k = a.shape
    buf = torch.full((m, k + 8), float('nan'), dtype=dtype, device='cuda')
    buf[:, :k] = a.cuda().to(dtype)
    return buf


def _checked(a, w, bias, family, step):
    """The preconditions of one GEMM case; returns the exact reference."""
    X.assert_operand(a, family == 'frac_a')
    X.assert_operand(w, family == 'frac_w')
    ref, bound = X.linear_ref(a, w, bias)
    X.assert_exact(bound, step)
    return ref


def _linear_fwd(a_buf, a_type, wp, planes, bias_d, c_type, m, n, k):
    """amtx_linear_fwd into a C with ldc = N + 8; the pad columns must still be zero afterwards."""
    ldc = n + 8
    c = torch.zeros(m, ldc, dtype=torch.float32 if c_type == F32 else torch.bfloat16, device='cuda')
    _lib.check(_lib.lib().amtx_linear_fwd(_lib.ptr(a_buf), a_buf.stride(0), a_type, _lib.ptr(wp), planes, _lib.ptr(bias_d), _lib.ptr(c), ldc, c_type,
                                          m, n, k, _stream()), 'amtx_linear_fwd')
    assert torch.all(c[:, n:] == 0)
    return c[:, :n].cpu()


@pytest.mark.parametrize('route,m,n,k', X.LINEAR_SHAPES, ids=_ids(X.LINEAR_SHAPES))
def test_linear_bf16_operands(route, m, n, k):
    """amtx_linear_fwd, bf16 A, one weight plane: the four direct-to-LDS kernels and the generic one, fp32 and bf16 C; then the same
    product from an fp32 A (rounded to bf16 by the generic kernel's loader: the same values)."""
    a, w, bias, step = X.linear_inputs(m, n, k, 'int', bias_max=640)
    ref = _checked(a, w, bias, 'int', step)
    rounded, ties = X.rounding_profile(ref)
    assert ref.numel() < 1000 or (rounded > 0 and ties > 0)                          # the bf16 C below has something to round, ties too
    wp, bias_d = _pack_linear(w, 1), bias.cuda()
    a16 = _padded(a, torch.bfloat16)
    assert _route(BF16, 1, F32, m, n, k, k + 8, n + 8) == route
    assert _route(BF16, 1, BF16, m, n, k, k + 8, n + 8) == ('GLDS128' if route == 'SKINNY' else route)     # (the skinny kernel writes fp32 only)
    assert torch.equal(_linear_fwd(a16, BF16, wp, 1, bias_d, F32, m, n, k), ref)
    assert torch.equal(_linear_fwd(a16, BF16, wp, 1, bias_d, BF16, m, n, k), ref.bfloat16())
    a32 = _padded(a, torch.float32)
    assert torch.equal(_linear_fwd(a32, F32, wp, 1, bias_d, F32, m, n, k), ref)
    assert torch.equal(_linear_fwd(a32, F32, wp, 1, bias_d, BF16, m, n, k), ref.bfloat16())


@pytest.mark.parametrize('family', ['frac_a', 'frac_w'])
@pytest.mark.parametrize('route,m,n,k', X.LINEAR_SHAPES, ids=_ids(X.LINEAR_SHAPES))
def test_linear_f32_a_two_plane_weights(route, m, n, k, family):
    """amtx_linear_fwd, fp32 A split in the loader, two weight planes (the generic kernel): each side fractional in turn."""
    a, w, bias, step = X.linear_inputs(m, n, k, family)
    ref = _checked(a, w, bias, family, step)
    got = _linear_fwd(_padded(a, torch.float32), F32, _pack_linear(w, 2), 2, bias.cuda(), F32, m, n, k)
    assert torch.equal(got, ref)


@pytest.mark.parametrize('family', ['int', 'frac_a', 'frac_w'])
@pytest.mark.parametrize('route,m,n,k', X.SPLIT_SHAPES, ids=_ids(X.SPLIT_SHAPES))
def test_linear_two_plane_a(route, m, n, k, family):
    """amtx_split_planes + amtx_linear_fwd_split: gemm_split_kernel, gemm_skinny_split_kernel and the generic kernel's split-A loader, fp32
    and two-plane C."""
    L = _lib.lib()
    a, w, bias, step = X.linear_inputs(m, n, k, family)
    ref = _checked(a, w, bias, family, step)
    wp, bias_d = _pack_linear(w, 2), bias.cuda()
    a32 = _padded(a, torch.float32)
    lda, ldc = k + 8, n + 8
    planes = torch.full((2, m, lda), NAN16, dtype=torch.int16, device='cuda')
    _lib.check(L.amtx_split_planes(_lib.ptr(a32), a32.stride(0), k, _lib.ptr(planes), lda, m * lda, m, _stream()), 'amtx_split_planes')
    hi, lo = X.split_bf16(a)
    assert torch.equal(X.planes_to_f32(planes[0, :, :k]).cpu(), hi) and torch.equal(X.planes_to_f32(planes[1, :, :k]).cpu(), lo)
    assert torch.all(planes[:, :, k:] == 0)                                         # amtx_split_planes zeroes columns k .. lda (include/amtx.h) ...
    planes[:, :, k:] = NAN16                                                         # ... so the canaries go in behind it: no GEMM may read them
    assert _route(SPLIT, 2, F32, m, n, k, lda, ldc) == route
    assert _route(SPLIT, 2, SPLIT, m, n, k, lda, ldc) == ('GENERIC' if route == 'SKINNY_SPLIT' else route)
    c = torch.zeros(m, ldc, device='cuda')
    _lib.check(L.amtx_linear_fwd_split(_lib.ptr(planes), lda, m * lda, _lib.ptr(wp), _lib.ptr(bias_d), _lib.ptr(c), ldc, F32, 0, m, n, k, _stream()),
               'amtx_linear_fwd_split')
    assert torch.equal(c[:, :n].cpu(), ref)
    assert torch.all(c[:, n:] == 0)
    cs = torch.zeros(2, m, ldc, dtype=torch.int16, device='cuda')
    _lib.check(L.amtx_linear_fwd_split(_lib.ptr(planes), lda, m * lda, _lib.ptr(wp), _lib.ptr(bias_d), _lib.ptr(cs), ldc, SPLIT, m * ldc, m, n, k,
                                       _stream()), 'amtx_linear_fwd_split (two-plane C)')
    chi, clo = X.split_bf16(ref)                                                     # bf16(c) and bf16(c - hi) of the exact c
    assert torch.equal(X.planes_to_f32(cs[0, :, :n]).cpu(), chi) and torch.equal(X.planes_to_f32(cs[1, :, :n]).cpu(), clo)
    assert torch.all(cs[:, :, n:] == 0)


# ---- inference convolutions: conv + folded BatchNorm + ReLU + MaxPool(1, 2), channels-last ----
# The kernels fuse ReLU and the pool, so these outputs are compared BEHIND them: an error in one pre-activation shows only where that value
# is positive and wins its pool pair.  A shift of up to 500 keeps most pre-activations positive, and an error of the kernel's indexing or
# tap loop touches a whole row of positions and channels, some of which always surface; one wrong (position, channel) term alone could hide.

def _conv_case(entry, b, t, f, cin, cout, planes, family):
    L = _lib.lib()
    x, w, scale, shift, step = X.conv_inputs(b, t, f, cin, cout, family)
    ws = w * scale[:, None, None, None]
    for v, frac in ((x, family == 'frac_a'), (ws, family == 'frac_w')):
        X.assert_splits(v, need_lo=v.numel() > 1000) if frac else X.assert_bf16(v)
    ref, bound = X.conv_ref(x, w, shift, scale)
    X.assert_exact(bound, step)
    ref = F.max_pool2d(F.relu(ref), (1, 2)).permute(0, 2, 3, 1).contiguous()         # (B, T, F / 2, Co)
    if entry == 'conv3x3':
        packed = np.zeros(L.amtx_conv3x3_packed_elems(cout, planes), dtype=np.uint16)
        _lib.check(L.amtx_conv3x3_pack(_lib.ptr(w.numpy()), _lib.ptr(scale.numpy()), cout, planes, _lib.ptr(packed)))
    else:
        nel = L.amtx_conv3x3g_packed_elems(cin, cout, planes)
        assert nel > 0
        packed = np.zeros(nel, dtype=np.uint16)
        _lib.check(L.amtx_conv3x3g_pack(_lib.ptr(w.numpy()), _lib.ptr(scale.numpy()), cin, cout, planes, _lib.ptr(packed)))
    wp = torch.from_numpy(packed.view(np.int16)).cuda()
    dtype = torch.bfloat16 if planes == 1 else torch.float32
    x_d = x.permute(0, 2, 3, 1).contiguous().cuda().to(dtype)
    out = torch.full((b, t, f // 2, cout), -7.0, dtype=dtype, device='cuda')         # (no output is negative behind the ReLU)
    shift_d = shift.cuda()
    if entry == 'conv3x3':
        _lib.check(L.amtx_conv3x3_fwd(_lib.ptr(x_d), BF16 if planes == 1 else F32, _lib.ptr(wp), planes, _lib.ptr(shift_d), _lib.ptr(out), b, t, f, cout,
                                      _stream()), 'amtx_conv3x3_fwd')
    else:
        _lib.check(L.amtx_conv3x3g_fwd(_lib.ptr(x_d), BF16 if planes == 1 else F32, _lib.ptr(wp), planes, _lib.ptr(shift_d), _lib.ptr(out), b, t, f, cin,
                                       cout, _stream()), 'amtx_conv3x3g_fwd')
    assert torch.equal(out.cpu(), ref.to(dtype)), (family, planes)                   # band edges, first and last frame of each clip included
    return ref


CONV_FAMILIES = {1: ('int', 'int_pos'), 2: ('int', 'int_pos', 'frac_w', 'frac_a')}


# amtx_conv3x3_fwd runs conv.hip's conv3x3_kernel for bf16 and for fp32 maps (convx.hip's kernels take two-plane maps, which only the
# engine builds: they are not reachable from an op-level entry point)
@pytest.mark.parametrize('planes', [1, 2])
@pytest.mark.parametrize('cout', [32, 64])
@pytest.mark.parametrize('b,t,f', X.CONV_SHAPES)
def test_conv3x3(b, t, f, cout, planes):
    for family in CONV_FAMILIES[planes]:
        ref = _conv_case('conv3x3', b, t, f, 32, cout, planes, family)
        if planes == 1 and ref.numel() > 2000:
            rounded, ties = X.rounding_profile(ref)
            assert rounded > ties > 0                                                # the bf16 output had something to round, ties and others


@pytest.mark.parametrize('planes', [1, 2])
@pytest.mark.parametrize('cin,cout', [(32, 32), (48, 48), (48, 96), (64, 64), (64, 128), (80, 80), (80, 160)])
@pytest.mark.parametrize('b,t,f', X.CONV_SHAPES)
def test_conv3x3_general_channels(b, t, f, cin, cout, planes):
    for family in CONV_FAMILIES[planes]:
        _conv_case('conv3x3g', b, t, f, cin, cout, planes, family)


@pytest.mark.parametrize('family', ['int', 'frac_a'])
@pytest.mark.parametrize('cin,f', [(1, 229), (6, 72)])
@pytest.mark.parametrize('layout', ['bcft', 'bctf'])
def test_conv1(cin, f, layout, family):
    """amtx_conv1_fwd: direct fp32 arithmetic (fused multiply-adds), fp32 and bf16 output."""
    L = _lib.lib()
    b, t, cout = 2, 19, 32
    x, w, _, shift, step = X.conv_inputs(b, t, f, cin, cout, family)                # x (B, C, T, F)
    ref, bound = X.conv_ref(x, w, shift)
    X.assert_exact(bound, 1.0 if family == 'int' else step * 2)                     # (no BatchNorm scale in this layer)
    ref = F.relu(ref).permute(0, 2, 3, 1).contiguous()
    xd = x.transpose(-1, -2).contiguous().cuda()                                    # the reference's (B, C, F, T)
    if layout == 'bctf':
        xd = xd.transpose(-1, -2).contiguous().transpose(-1, -2)
    sb, sc, sf, st = xd.stride()
    w_d, shift_d = w.cuda(), shift.cuda()
    for out_type, dtype in ((F32, torch.float32), (BF16, torch.bfloat16)):
        out = torch.full((b, t, f, cout), -7.0, dtype=dtype, device='cuda')
        _lib.check(L.amtx_conv1_fwd(_lib.ptr(xd), sb, sc, st, sf, _lib.ptr(w_d), _lib.ptr(shift_d), _lib.ptr(out), out_type, b, t, f, cin, cout,
                                    _stream()), 'amtx_conv1_fwd')
        assert torch.equal(out.cpu(), ref.to(dtype))


# ---- training GEMMs (train.hip): fp32 operands split inside the kernels ----

@pytest.mark.parametrize('a_trans', [False, True])
@pytest.mark.parametrize('b_trans', [False, True])
@pytest.mark.parametrize('shape,family', X.MATMUL_CASES, ids=lambda v: str(v).replace(' ', ''))
def test_matmul_f32(shape, family, a_trans, b_trans):
    """amtx_matmul_f32 (xgemm): every operand orientation, with and without bias and split contraction, a padded C."""
    L = _lib.lib()
    M, N, K = shape
    if a_trans:
        M += (-M) % 4                                                                # the contiguous extent of a transposed operand is a multiple of 4
    a, b, bias, step = X.matmul_inputs(M, N, K, family)
    X.assert_operand(a, family == 'frac_a')
    X.assert_operand(b, family == 'frac_b')
    ref, bound = X.linear_ref(a, b, bias)
    X.assert_exact(bound, step)
    ref0 = ref - bias                                                                # (exact: both on the grid, below the bound)
    a_d = (a.T.contiguous() if a_trans else a).cuda()
    b_d = (b.T.contiguous() if b_trans else b).cuda()
    bias_d = bias.cuda()
    need = int(L.amtx_matmul_workspace_bytes(M, N, K))
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device='cuda')
    for with_bias in (False, True):
        c = torch.zeros(M, N, device='cuda')
        _lib.check(L.amtx_matmul_f32(_lib.ptr(a_d), a_d.stride(0), int(a_trans), _lib.ptr(b_d), b_d.stride(0), int(b_trans), _lib.ptr(bias_d) if with_bias else None,
                                     _lib.ptr(c), N, M, N, K, _lib.ptr(ws), ws.numel(), _stream()), 'amtx_matmul_f32')
        assert torch.equal(c.cpu(), ref if with_bias else ref0)
    cpad = torch.zeros(M, N + 4, device='cuda')                                      # ldc != n: no split contraction
    _lib.check(L.amtx_matmul_f32(_lib.ptr(a_d), a_d.stride(0), int(a_trans), _lib.ptr(b_d), b_d.stride(0), int(b_trans), _lib.ptr(bias_d), _lib.ptr(cpad), N + 4,
                                 M, N, K, None, 0, _stream()), 'amtx_matmul_f32 (padded C)')
    assert torch.equal(cpad[:, :N].cpu(), ref) and torch.all(cpad[:, N:] == 0)


def _train_cases(shapes, frac_shape):
    return [(s, fam) for s in shapes for fam in X.TRAIN_FAMILIES if fam == 'int' or s == frac_shape]


@pytest.mark.parametrize('shape,family', _train_cases(X.TRAIN_LINEAR_SHAPES, X.TRAIN_LINEAR_FRAC_SHAPE), ids=lambda v: str(v).replace(' ', ''))
def test_autograd_linear(shape, family):
    from amt_tools_amd.autograd import linear
    m, n, k = shape
    x, w, bias, dy, step = X.train_operands((m, k), (n, k), (m, n), n, family, shape)
    for v, name in ((x, 'frac_x'), (w, 'frac_w'), (dy, 'frac_dy')):
        X.assert_operand(v, family == name)
    refs = X.train_linear_refs(x, w, bias, dy)
    for _, bound in refs.values():
        X.assert_exact(bound, step)
    xc, wc, bc = (v.cuda().requires_grad_(True) for v in (x, w, bias))
    y = linear(xc, wc, bc)
    y.backward(dy.cuda())
    for name, got in (('y', y.detach()), ('dx', xc.grad), ('dw', wc.grad), ('db', bc.grad)):
        assert torch.equal(got.cpu(), refs[name][0]), name


@pytest.mark.parametrize('ci,co', X.TRAIN_CONV_CHANNELS)
@pytest.mark.parametrize('shape,family', _train_cases(X.TRAIN_CONV_SHAPES, X.TRAIN_CONV_FRAC_SHAPE), ids=lambda v: str(v).replace(' ', ''))
def test_autograd_conv3x3(shape, family, ci, co):
    from amt_tools_amd.autograd import conv3x3
    b, t, f = shape
    x, w, bias, dy, step = X.train_operands((b, ci, t, f), (co, ci, 3, 3), (b, co, t, f), co, family, shape + (ci, co))
    for v, name in ((x, 'frac_x'), (w, 'frac_w'), (dy, 'frac_dy')):
        X.assert_operand(v, family == name)
    refs = X.train_conv_refs(x, w, bias, dy)
    for _, bound in refs.values():
        X.assert_exact(bound, step)
    conv = torch.nn.Conv2d(ci, co, 3, padding=1).cuda()
    conv.load_state_dict({'weight': w, 'bias': bias})
    xc = x.cuda().contiguous(memory_format=torch.channels_last).requires_grad_(ci > 1)   # (the one-channel first layer has no input gradient)
    y = conv3x3(xc, conv)
    y.backward(dy.cuda())
    results = [('y', y.detach()), ('dw', conv.weight.grad), ('db', conv.bias.grad)] + ([('dx', xc.grad)] if ci > 1 else [])
    for name, got in results:
        assert torch.equal(got.cpu(), refs[name][0]), name
