"""tests/exact_inputs.py on the CPU: the operands of the exact GPU tests (tests/test_gpu_exact.py) meet their conditions at every shape
that file uses, fp32 arithmetic in different k-orders returns the reference's bits (so the reference alone stays within the conditions),
and a product with one dropped term or one swapped pair of weight columns does not."""
import pytest

torch = pytest.importorskip('torch')
import torch.nn.functional as F   # noqa: E402

import exact_inputs as X          # noqa: E402

LINEAR_CASES = [(m, n, k, fam) for _, m, n, k in X.LINEAR_SHAPES for fam in ('int', 'frac_a', 'frac_w')]
SPLIT_CASES = [(m, n, k, fam) for _, m, n, k in X.SPLIT_SHAPES for fam in ('int', 'frac_a', 'frac_w')]


def _check_operands(a, w, family, frac_name_a='frac_a', frac_name_w='frac_w'):
    for t, frac in ((a, family == frac_name_a), (w, family == frac_name_w)):
        assert (t != 0).all()
        if frac:
            X.assert_splits(t, need_lo=t.numel() > 1000)
        else:
            X.assert_bf16(t)


@pytest.mark.parametrize('m,n,k,family', sorted(set(LINEAR_CASES + SPLIT_CASES)))
def test_linear_operands_meet_the_conditions_and_fp32_is_exact_in_any_order(m, n, k, family):
    a, w, bias, step = X.linear_inputs(m, n, k, family)
    _check_operands(a, w, family)
    ref, bound = X.linear_ref(a, w, bias)
    X.assert_exact(bound, step)
    if m * n * k > 3e8:
        a, ref = a[:256], ref[:256]                                   # (the k-order checks below on a slice of the tall problems)
    assert torch.equal(F.linear(a, w, bias), ref)                     # fp32, the BLAS's order
    hi, lo = X.split_bf16(a)
    whi, wlo = X.split_bf16(w)
    perm = torch.randperm(k, generator=X.gen(k))
    c = bias.expand(a.shape[0], n).clone()                            # the three-product sum, k permuted and in chunks, last chunk first
    for ks in reversed(torch.split(perm, 40)):
        c = c + hi[:, ks] @ wlo[:, ks].T
        c = c + lo[:, ks] @ whi[:, ks].T
        c = c + hi[:, ks] @ whi[:, ks].T
    assert torch.equal(c, ref)


def test_bf16_output_references_hold_rounded_values_and_ties():
    """Outputs that bf16 changes, and ties among them, exist in the cases the GPU file counts on (bias up to 640 puts outputs of every K
    into [256, 512), where the odd integers are ties, and beyond, where three integers in four need rounding)."""
    for _, m, n, k in X.LINEAR_SHAPES:
        a, w, bias, _ = X.linear_inputs(min(m, 300), n, k, 'int', bias_max=640)
        ref, bound = X.linear_ref(a, w, bias)
        X.assert_exact(bound)
        rounded, ties = X.rounding_profile(ref)
        if ref.numel() >= 1000:
            assert rounded > 0 and ties > 0 and (rounded > ties or n == 4), (m, n, k, rounded, ties)   # (N = 4: four bias values)
    ref = torch.tensor([255.0, 256.0, 257.0, 258.0, 259.0, 513.0, 514.0, 515.0, 0.5, 128.5])
    assert X.rounding_profile(ref) == (6, 4)                          # 257, 259, 514 and 128.5 are ties; 513 and 515 round without one
    assert torch.equal(ref.bfloat16().float(), torch.tensor([255.0, 256.0, 256.0, 258.0, 260.0, 512.0, 512.0, 516.0, 0.5, 128.0]))


@pytest.mark.parametrize('family', ['int', 'frac_a', 'frac_w'])
def test_a_corrupted_product_is_not_the_reference(family):
    m, n, k = 257, 88, 256
    a, w, bias, _ = X.linear_inputs(m, n, k, family)
    ref, _ = X.linear_ref(a, w, bias)
    dropped = a.clone()
    dropped[200, k - 1] = 0                                           # ONE term of one row dropped
    got = F.linear(dropped, w, bias)
    assert not torch.equal(got[200], ref[200]) and (got[200] != ref[200]).all() and torch.equal(got[:200], ref[:200])
    swapped = w.clone()
    swapped[:, [70, 71]] = w[:, [71, 70]]                             # one pair of weight columns (k-lanes) swapped
    got = F.linear(a, swapped, bias)
    wrong = (got != ref).float().mean().item()
    assert wrong > 0.3, wrong                                         # (a_70 - a_71)(w_70 - w_71) != 0 for most (row, column) pairs
    if family == 'frac_a':                                            # the smallest error the split arithmetic can make: one low-plane term lost
        lo = X.split_bf16(a)[1]
        j = int(torch.nonzero(lo[5])[0])
        no_lo = a.clone()
        no_lo[5, j] -= lo[5, j]
        assert (F.linear(no_lo, w, bias)[5] != ref[5]).all()


CONV_CASES = [(b, t, f, ci, co) for b, t, f in X.CONV_SHAPES for ci, co in ((32, 64), (80, 160), (6, 32))]


@pytest.mark.parametrize('b,t,f,ci,co', CONV_CASES)
def test_conv_operands_meet_the_conditions(b, t, f, ci, co):
    """(32 -> 64: conv.hip's widest layer; 80 -> 160: convg.hip's longest contraction, 720 terms; 6 -> 32: the first layer)"""
    for family in ('int', 'int_pos', 'frac_w', 'frac_a'):
        x, w, scale, shift, step = X.conv_inputs(b, t, f, ci, co, family)
        ws = w * scale[:, None, None, None]                           # what the pack computes, in fp32
        assert torch.equal(ws.double(), w.double() * scale.double()[:, None, None, None])
        _check_operands(x, ws, family)
        assert family != 'int_pos' or (x > 0).all()
        ref, bound = X.conv_ref(x, w, shift, scale)
        X.assert_exact(bound, step)
        assert torch.equal(F.conv2d(x, ws, shift, padding=1), ref)
        if family.startswith('int') and ref.numel() > 4000 and ci >= 32:  # (what the bf16 maps of conv.hip and convg.hip have to round)
            rounded, ties = X.rounding_profile(F.max_pool2d(F.relu(ref), (1, 2)))
            assert rounded > ties > 0


@pytest.mark.parametrize('family', X.TRAIN_FAMILIES)
def test_training_linear_operands_and_the_largest_fractional_shape(family):
    size = lambda s: s[0] * s[1] * s[2]
    for shape in X.TRAIN_LINEAR_SHAPES:
        m, n, k = shape
        x, w, bias, dy, step = X.train_operands((m, k), (n, k), (m, n), n, family, shape)
        _check_operands(x, w, family, 'frac_x', 'frac_w')
        _check_operands(dy, w, family, 'frac_dy', 'frac_w')
        refs = X.train_linear_refs(x, w, bias, dy)
        fits = all(float(bound.max()) / step <= X.LIMIT for _, bound in refs.values())
        if family == 'int' or shape == X.TRAIN_LINEAR_FRAC_SHAPE:
            assert fits, shape                                        # the integer family runs every shape, the others the largest
        assert size(shape) <= size(X.TRAIN_LINEAR_FRAC_SHAPE)
        if fits and size(shape) < 1e8:
            assert torch.equal(F.linear(x, w, bias), refs['y'][0]) and torch.equal(dy @ w, refs['dx'][0])
            assert torch.equal(dy.T @ x, refs['dw'][0]) and torch.equal(dy.sum(0), refs['db'][0])


@pytest.mark.parametrize('ci,co', X.TRAIN_CONV_CHANNELS)
@pytest.mark.parametrize('family', X.TRAIN_FAMILIES)
def test_training_conv_operands_and_the_largest_fractional_shape(family, ci, co):
    size = lambda s: s[0] * s[1] * s[2]
    for shape in X.TRAIN_CONV_SHAPES:
        if family != 'int' and size(shape) > 4 * size(X.TRAIN_CONV_FRAC_SHAPE):
            continue                                                  # (3, 64, 229): 13 times the positions of a shape that already fails
        b, t, f = shape
        x, w, bias, dy, step = X.train_operands((b, ci, t, f), (co, ci, 3, 3), (b, co, t, f), co, family, shape + (ci, co))
        for v, name in ((x, 'frac_x'), (w, 'frac_w'), (dy, 'frac_dy')):
            X.assert_operand(v, family == name)
        refs = X.train_conv_refs(x, w, bias, dy)
        fits = all(float(bound.max()) / step <= X.LIMIT for _, bound in refs.values())
        if family == 'int' or size(shape) <= size(X.TRAIN_CONV_FRAC_SHAPE):
            assert fits, shape
        elif family != 'frac_w':                                      # (the weight gradient has no fractional operand in 'frac_w')
            assert not fits, shape
        if fits and size(shape) <= size(X.TRAIN_CONV_FRAC_SHAPE):
            xg, wg = x.clone().requires_grad_(True), w.clone().requires_grad_(True)
            bg = bias.clone().requires_grad_(True)
            y = F.conv2d(xg, wg, bg, padding=1)
            y.backward(dy)
            for name, got in (('y', y.detach()), ('dx', xg.grad), ('dw', wg.grad), ('db', bg.grad)):
                assert torch.equal(got, refs[name][0]), (shape, name)


_KERNEL_ROUTES = (('gemm_skinny_split_kernel', 'SKINNY_SPLIT'), ('gemm_skinny_kernel', 'SKINNY'), ('gemm_split_kernel', 'SPLIT'), ('gemm_pp_kernel', 'PP'),
                  ('gemm_glds_kernel<0, 128>', 'GLDS128'), ('gemm_glds_kernel<1, 128>', 'GLDS128'), ('gemm_glds_kernel<0, 256>', 'GLDS256'),
                  ('gemm_glds_kernel<1, 256>', 'GLDS256'), ('gemm_kernel<', 'GENERIC'))


def test_route_mirror_answers_what_the_library_launches():
    """exact_inputs.route against the LIBRARY's routing: tests/golden/launch_trace.json holds the kernel that amtx_linear_fwd /
    amtx_linear_fwd_split launch for 15876 problems (tests/test_sanitized_host.py requires the present gemm.hip to reproduce every row of
    it), so a threshold that moves in gemm_route either fails that test or, once the trace is re-recorded, this one.  Every problem the
    library takes, in the type combinations the exact tests use, both sides of every threshold of M, N, K and lda."""
    import json
    import os
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.join(here, 'san'))
    import launch_trace
    with open(os.path.join(here, 'golden', 'launch_trace.json')) as f:
        rows = iter(launch_trace.expand(json.load(f))['']['gemm'])
    M, N, K = (1, 255, 256, 1023, 1024, 4096), (4, 88, 128, 256, 512, 1024, 2048), (8, 64, 128, 176, 192, 512, 1024, 1088, 3648)   # tests/san/driver.py: trace_gemm
    checked = {}
    for m in M:
        for n in N:
            for k in K:
                for lda in (k, k + 8):
                    calls = [(a, c, p) for a in (0, 1, 2) for c in (0, 1, 2) for p in (1, 2)] + [(X.SPLIT, c, 2) for c in (0, 1, 2)]
                    for i, (a_type, c_type, planes) in enumerate(calls):
                        rc, _, launches = next(rows)
                        used = (a_type in (X.BF16, X.F32) and c_type in (X.BF16, X.F32)) if i < 18 else c_type in (X.F32, X.SPLIT)
                        if rc != 0 or not used:
                            continue
                        assert len(launches) == 1
                        got = next(r for name, r in _KERNEL_ROUTES if name in launches[0])
                        assert X.route(a_type, planes, c_type, m, n, k, lda, n) == got, (a_type, planes, c_type, m, n, k, lda, launches[0])
                        checked[got] = checked.get(got, 0) + 1
    assert next(rows, None) is None
    assert set(checked) == {'SKINNY', 'SKINNY_SPLIT', 'GLDS128', 'GLDS256', 'PP', 'SPLIT', 'GENERIC'} and min(checked.values()) >= 20, checked


def test_route_mirror_names_the_shapes_as_listed():
    for name, m, n, k in X.LINEAR_SHAPES:
        assert X.route(X.BF16, 1, X.F32, m, n, k, k + 8, n + 8) == name, (name, m, n, k)
        assert X.route(X.BF16, 1, X.BF16, m, n, k, k + 8, n + 8) == ('GLDS128' if name == 'SKINNY' else name), (name, m, n, k)
        assert X.route(X.F32, 1, X.F32, m, n, k, k + 8, n + 8) == 'GENERIC'
    for name, m, n, k in X.SPLIT_SHAPES:
        assert X.route(X.SPLIT, 2, X.F32, m, n, k, k + 8, n + 8) == name, (name, m, n, k)
        assert X.route(X.SPLIT, 2, X.SPLIT, m, n, k, k + 8, n + 8) == ('GENERIC' if name == 'SKINNY_SPLIT' else name), (name, m, n, k)
    assert {r for r, *_ in X.LINEAR_SHAPES} == {'SKINNY', 'GLDS128', 'GLDS256', 'PP', 'GENERIC'}
    assert {r for r, *_ in X.SPLIT_SHAPES} == {'SPLIT', 'SKINNY_SPLIT', 'GENERIC'}


@pytest.mark.parametrize('family', ['int', 'frac_a', 'frac_b'])
def test_matmul_operands_meet_the_conditions(family):
    for shape in X.MATMUL_SHAPES:
        a, b, bias, step = X.matmul_inputs(*shape, family)
        X.assert_operand(a, family == 'frac_a')
        X.assert_operand(b, family == 'frac_b')
        ref, bound = X.linear_ref(a, b, bias)
        fits = float(bound.max()) / step <= X.LIMIT
        assert fits == (family == 'int' or shape in X.MATMUL_FRAC_SHAPES), shape
        if fits:
            assert torch.equal(F.linear(a, b, bias), ref)
