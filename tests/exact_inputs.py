"""Operands on an integer grid for the exact GPU tests (tests/test_gpu_exact.py): with them a kernel whose arithmetic is only multiply and
add has ONE right answer, bit for bit, whatever its tiling, k-order or split contraction -- and that answer is a float64 product.

Three things hold for the operands made here (tests/test_exact_inputs.py proves them on the CPU, at every shape the GPU file uses):
1. every operand is exactly what the kernel feeds the matrix cores: representable in bf16 (`assert_bf16`), or, for the split-bf16 ('x3')
   paths, equal to hi + lo with hi = bf16(x), lo = bf16(x - hi) (`assert_splits`);
2. every product is exact in fp32 (two operands of at most 8 + 8 significant bits);
3. every partial sum, in any order, is exact in fp32: `assert_exact` takes sum_k |a||w| + |bias| (the largest magnitude any partial sum of
   any order can reach), divides it by the grid step (the spacing of the products: 1 for integers, 2^-s for a fractional operand) and
   requires at most LIMIT = 2^21 steps -- three bits under the 2^24 consecutive integers of an fp32 significand.

THE HEADROOM IS AN ASSUMPTION.  The three bits are there because how the bf16 matrix instructions accumulate internally had not been
measured before these tests existed (the programming guide documents only the fp32 instruction as a chain of fused multiply-adds); an
accumulator that keeps fewer low bits than fp32 would show up as a failure that goes away when the operand magnitudes are halved.

Two operand families:
* `integers`: values from a set WITHOUT zero, so no product vanishes and a dropped, doubled or mispaired term moves an output by at
  least one grid step;
* `fractional`: p + q / 2^s with p from such a set and q in -qmax .. qmax: more than 8 significant bits when q is odd, i.e. a non-zero low
  plane under the bf16 split.  ONE-SIDED RULE: only one operand of a product is fractional, the other is an integer (lo = 0), so the
  lo.lo term that the split arithmetic drops (hi.hi + hi.lo + lo.hi) is identically zero and the reference is the TRUE product, not a
  model of what the kernel keeps.

bf16 results: the expected output of a kernel that writes bf16 (or two planes) is the exact value rounded ONCE, `.bfloat16()` = round to
nearest even; `rounding_profile` counts the outputs that need rounding and the ties among them (odd integers in [256, 512) are ties)."""
import torch

LIMIT = 2 ** 21                      # grid steps sum |a||w| + |bias| may reach (fp32 holds 2^24)
INTS_A = (-3, -2, -1, 1, 2, 3)       # activations
INTS_A_POS = (1, 2, 3)               # non-negative activations (what a ReLU in front of a layer leaves)
INTS_W = (-2, -1, 1, 2)              # weights
SCALES = (0.5, 1.0, 2.0)             # folded BatchNorm scales: w * scale stays on the grid through the pack's fp32 multiply


FAMILIES = ('int', 'int_pos', 'frac_a', 'frac_w', 'frac_b', 'frac_x', 'frac_dy')     # every family name; its index seeds the generator


def gen(*seed):
    s = 0
    for v in seed:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def integers(shape, values, g):
    """fp32 tensor of `shape`, every element drawn from `values`."""
    v = torch.tensor(values, dtype=torch.float32)
    return v[torch.randint(len(values), tuple(shape), generator=g)]


def fractional(shape, values, g, s=9, qmax=3):
    """p + q / 2^s, p from `values`, q uniform in -qmax .. qmax (exact in fp32: at most 2 + s significant bits)."""
    q = torch.randint(-qmax, qmax + 1, tuple(shape), generator=g).double()
    return (integers(shape, values, g).double() + q / 2.0 ** s).float()


def split_bf16(x):
    """(hi, lo) as fp32 values: hi = bf16(x), lo = bf16(x - hi), both round to nearest even -- the planes of the 'x3' arithmetic."""
    hi = x.bfloat16().float()
    return hi, (x - hi).bfloat16().float()


def assert_bf16(x):
    assert torch.equal(x.bfloat16().float(), x), 'operand is not representable in bf16'


def assert_splits(x, need_lo=False):
    hi, lo = split_bf16(x)
    assert torch.equal(hi.double() + lo.double(), x.double()), 'hi + lo != x'
    if need_lo:
        assert x.numel() < 1000 or (lo != 0).float().mean().item() > 0.1, 'the low plane is (nearly) empty: this operand does not test the split'


def assert_operand(x, fractional_family):
    """Condition 1 for one operand: hi + lo == x with a populated low plane (fractional), or bf16 itself (integer); never zero."""
    assert (x != 0).all()
    assert_splits(x, need_lo=True) if fractional_family else assert_bf16(x)


def assert_exact(bound, step=1.0):
    """`bound` = sum_k |a||w| + |bias| per output (float64).  The precondition of every exact test; asserted before any launch."""
    steps = float(bound.max()) / step
    assert steps <= LIMIT, f'sum |a||w| + |bias| reaches {steps:.0f} grid steps of {step}: more than 2^21'
    return steps


def to_f32(ref64):
    """The float64 reference as fp32, which must lose nothing."""
    ref = ref64.float()
    assert torch.equal(ref.double(), ref64), 'reference is not representable in fp32'
    return ref


def linear_ref(a, w, bias=None):
    """(exact a w^T + bias as fp32, the magnitude bound sum |a||w| + |bias| as float64)."""
    ref = a.double() @ w.double().T
    bound = a.double().abs() @ w.double().abs().T
    if bias is not None:
        ref = ref + bias.double()
        bound = bound + bias.double().abs()
    return to_f32(ref), bound


def conv_ref(x_bcft, w, bias=None, scale=None):
    """3x3 convolution, zero padding 1, of x (B, C, T, F) with w (Co, C, 3, 3) * scale[Co] + bias[Co]: (exact fp32, magnitude bound)."""
    import torch.nn.functional as F
    wd = w.double() if scale is None else w.double() * scale.double()[:, None, None, None]
    ref = F.conv2d(x_bcft.double(), wd, None if bias is None else bias.double(), padding=1)
    bound = F.conv2d(x_bcft.double().abs(), wd.abs(), None if bias is None else bias.double().abs(), padding=1)
    return to_f32(ref), bound


def rounding_profile(ref):
    """(outputs whose bf16 rounding changes them, ties among those) of an fp32 reference."""
    low = ref.contiguous().view(torch.int32) & 0xFFFF
    return int((low != 0).sum()), int((low == 0x8000).sum())


def planes_to_f32(p):
    """An int16 plane of bf16 bit patterns as fp32 values."""
    return (p.to(torch.int32) << 16).view(torch.float32)


# ---- the GEMM shapes of tests/test_gpu_exact.py, by the route gemm.hip's gemm_route gives them ----
# Constants of gemm.hip: BM = BN = 128 (n_pad = N rounded up to 128); GBK = 64 (k_pad = K rounded up to 64; the direct-to-LDS kernels
# need K == k_pad); RBK = 32 (the ring needs K >= 4 RBK = 128 and K <= 1024); skinny: n_pad == 128, fp32 C, M >= 1024, K >= 2 GBK = 128
# (two-plane variant: K >= 2 RBK = 64); whole 256-tiles: N % 256 == 0 and M >= 256.
F32, BF16, SPLIT = 1, 0, 2


def route(a_type, planes, c_type, m, n, k, lda, ldc):
    """gemm_route in Python, for the arguments amtx_linear_fwd / amtx_linear_fwd_split build and no A/B switch set: the tests assert
    that every shape runs where its id says.  This is a COPY of the C++ decision, tied to it only through the CPU suite:
    tests/test_exact_inputs.py compares it with the kernel the library launches for each of the 15876 problems of
    tests/golden/launch_trace.json, which tests/test_sanitized_host.py holds the present gemm.hip to.  It knows no A/B switch: the GPU
    tests refuse to run with one of gemm.hip's switches in the environment."""
    n_pad, k_pad = -(-n // 128) * 128, -(-k // 64) * 64
    tiles256 = n % 256 == 0 and m >= 256
    if a_type == BF16 and planes == 1 and k == k_pad and lda % 8 == 0:
        if n_pad == 128 and c_type == F32 and m >= 1024 and k >= 128:
            return 'SKINNY'
        if not tiles256:
            return 'GLDS128'
        if 128 <= k <= 1024 and n_pad <= 4096 and (ldc * (4 if c_type == F32 else 2)) % 16 == 0:
            return 'PP'
        return 'GLDS256'
    if a_type == SPLIT:
        c_aligned = ldc % 8 == 0 if c_type == SPLIT else ldc % 4 == 0
        if tiles256 and k == k_pad and lda % 8 == 0 and c_aligned:
            return 'SPLIT'
        if n_pad == 128 and c_type == F32 and m >= 1024 and k == k_pad and k >= 64 and lda % 8 == 0:
            return 'SKINNY_SPLIT'
    return 'GENERIC'


# bf16 A, one weight plane (route with fp32 C; a bf16 C sends SKINNY to GLDS128, everything else stays)
LINEAR_SHAPES = [
    ('GLDS128', 1, 4, 64), ('GLDS128', 129, 132, 64), ('GLDS128', 257, 88, 192), ('GLDS128', 255, 256, 128),      # M = 255: no full row tile
    ('GLDS128', 1023, 88, 128), ('GLDS128', 1024, 88, 64), ('GLDS128', 1025, 132, 128),    # skinny's M >= 1024, K >= 128, n_pad == 128, from below
    ('GLDS256', 256, 256, 64), ('GLDS256', 257, 256, 1088), ('GLDS256', 300, 512, 3648),   # K = 64 < 128 and K = 1088 > 1024: not the ring
    ('PP', 256, 256, 128), ('PP', 300, 256, 192), ('PP', 385, 512, 1024),
    ('SKINNY', 1024, 4, 128), ('SKINNY', 1025, 88, 128), ('SKINNY', 2500, 128, 192), ('SKINNY', 4099, 88, 512),
    ('SKINNY', 33000, 88, 128),                                                            # 258 row tiles on 256 blocks
    ('SKINNY', 1300, 88, 3648),                                                            # (the pitch head's K: outputs that need bf16 rounding)
    ('GENERIC', 5, 88, 8), ('GENERIC', 130, 132, 40), ('GENERIC', 64, 1024, 176),          # K no multiple of 64
]
# two-plane A (amtx_split_planes), two weight planes.  K = 32, 96, 1056 are whole 32-deep stages but no multiple of 64 = k_pad's unit:
# the direct-to-LDS two-plane kernels refuse them and the generic kernel's split-A loader runs -- the other side of that threshold
SPLIT_SHAPES = [
    ('SPLIT', 256, 256, 64), ('SPLIT', 300, 512, 128), ('SPLIT', 257, 256, 1088),
    ('SKINNY_SPLIT', 1024, 4, 64), ('SKINNY_SPLIT', 1300, 88, 128), ('SKINNY_SPLIT', 4099, 128, 512),
    ('GENERIC', 256, 256, 32), ('GENERIC', 300, 512, 96), ('GENERIC', 257, 256, 1056),
    ('GENERIC', 1300, 88, 96), ('GENERIC', 1023, 88, 64),
    ('GENERIC', 5, 88, 8), ('GENERIC', 255, 256, 64), ('GENERIC', 1000, 88, 256), ('GENERIC', 300, 260, 72),
]


def frac_bits(k):
    """s of the fractional family for a contraction of length k: sum |a||w| is about 3 k (mean |a| = 2, mean |w| = 1.5) and has to stay
    under 2^21 2^-s: s = 9 up to k = 1100 (3 * 1100 * 512 = 2^20.7), s = 7 above (k = 3648: 3 * 3648 * 128 = 2^20.4).  From s = 7 on
    p = +-2, +-3 with an odd q has nine significant bits or more: a non-zero low plane.  assert_exact decides, not this estimate."""
    return 9 if k <= 1100 else 7


def linear_inputs(m, n, k, family, bias_max=8):
    """(a, w, bias, grid step) of one GEMM case.  family: 'int' | 'frac_a' | 'frac_w'."""
    g = gen(m, n, k, FAMILIES.index(family))
    s = frac_bits(k)
    a = fractional((m, k), INTS_A, g, s) if family == 'frac_a' else integers((m, k), INTS_A, g)
    w = fractional((n, k), INTS_W, g, s) if family == 'frac_w' else integers((n, k), INTS_W, g)
    bias = torch.randint(-bias_max, bias_max + 1, (n,), generator=g).float()
    return a, w, bias, (1.0 if family == 'int' else 2.0 ** -s)


# ---- convolution shapes (B, T, F); B T F stays under 20 000 positions ----
CONV_SHAPES = [
    (1, 1, 2), (3, 5, 36), (1, 33, 18), (2, 16, 33), (1, 17, 114),       # the small shapes of tests/test_gpu_ops.py
    (1, 16, 46),     # conv.hip: exactly one tile (TT = 16 frames, FT_MAX = 46 columns); convg.hip: GTT = 16, FT = 32 | 16 + a ragged tile
    (1, 17, 48),     # conv.hip: one frame past TT, two columns past FT_MAX (two 24-column tiles)
    (2, 16, 32),     # convg.hip: exactly one FT = 32 tile (bf16) / two FT = 16 tiles (two-plane)
    (1, 17, 34),     # convg.hip: one pooled column past FT = 32, one frame past GTT
    (1, 15, 16),     # convg.hip: exactly one FT = 16 tile of the two-plane kernel, one frame short of GTT
    (520, 1, 4),     # 520 tiles: more than the 512 blocks of conv.hip's persistent grid; one-frame clips (both time neighbours are padding)
]
# (convg.hip's strips -- SPW = 8 output columns, three per tile -- exist only in the kernel variants with a fused first conv (STRIP needs
# KS1 > 0), which the engine launches and amtx_conv3x3g_fwd does not: no shape here is tied to them.  The same holds for convx.hip's
# XFT = 30 / XT = 16 tiles and convf.hip's strips: two-plane maps and the fused stack are built by the engine only.)


def conv_inputs(b, t, f, cin, cout, family, s=7):
    """(x (B, C, T, F), w, scale, shift, grid step).  family: 'int' | 'int_pos' | 'frac_w' | 'frac_a'.  s = 7: with 9 c_in <= 720 terms of
    mean |x| |w| scale = 2 * 1.5 * 1.17 the sum is about 2500 = 2^11.3; times 2^7, times 2 for scale = 0.5: 2^19.3."""
    g = gen(b, t, f, cin, cout, FAMILIES.index(family))
    x = fractional((b, cin, t, f), INTS_A, g, s) if family == 'frac_a' else integers((b, cin, t, f), INTS_A_POS if family == 'int_pos' else INTS_A, g)
    w = fractional((cout, cin, 3, 3), INTS_W, g, s) if family == 'frac_w' else integers((cout, cin, 3, 3), INTS_W, g)
    scale = integers((cout,), SCALES, g)
    shift = torch.randint(-100, 501, (cout,), generator=g).float()     # up to 500: outputs in [256, 512) and beyond, which a bf16 map has to round
    return x, w, scale, shift, (0.5 if family.startswith('int') else 2.0 ** -(s + 1))


# ---- training GEMMs (train.hip): fp32 operands that the kernels split themselves; three products share three operands ----
# y = x w^T + b, dx = dy w, dW = dy^T x, db = column sums of dy.  One-sided rule: ONE of x, w, dy is fractional per family.
TRAIN_FAMILIES = ('int', 'frac_x', 'frac_w', 'frac_dy')
TRAIN_S = 7          # 2^21 2^-7 = 16384: contractions of up to ~4000 terms of mean |x||dy| = 4 (the weight gradients sum over rows / positions)
TRAIN_LINEAR_SHAPES = [(1, 4, 4), (37, 88, 256), (625, 512, 3648), (5000, 88, 512), (130, 1024, 176), (4999, 132, 36)]   # tests/test_gpu_train.py
TRAIN_LINEAR_FRAC_SHAPE = (625, 512, 3648)      # the largest (M N K) of them whose four results meet assert_exact (tests/test_exact_inputs.py)
TRAIN_CONV_CHANNELS = [(1, 32), (16, 16), (32, 64), (48, 96)]
TRAIN_CONV_SHAPES = [(1, 1, 2), (2, 7, 13), (3, 20, 57), (1, 33, 229), (3, 64, 229)]      # (3, 64, 229): several wgrad steps per block
TRAIN_CONV_FRAC_SHAPE = (3, 20, 57)             # likewise: 3420 positions in the weight gradient's contraction


def train_operands(shape_x, shape_w, shape_dy, n_bias, family, seed):
    g = gen(*seed, FAMILIES.index(family))
    mk = lambda shape, frac: fractional(shape, INTS_A, g, TRAIN_S) if frac else integers(shape, INTS_A, g)
    x = mk(shape_x, family == 'frac_x')
    w = fractional(shape_w, INTS_W, g, TRAIN_S) if family == 'frac_w' else integers(shape_w, INTS_W, g)
    dy = mk(shape_dy, family == 'frac_dy')
    bias = torch.randint(-8, 9, (n_bias,), generator=g).float()
    return x, w, bias, dy, (1.0 if family == 'int' else 2.0 ** -TRAIN_S)


def train_linear_refs(x, w, bias, dy):
    """{name: (exact fp32, magnitude bound)} of autograd.linear's four results."""
    return {'y': linear_ref(x, w, bias), 'dx': linear_ref(dy, w.T.contiguous()), 'dw': linear_ref(dy.T.contiguous(), x.T.contiguous()),
            'db': (to_f32(dy.double().sum(0)), dy.double().abs().sum(0))}


def train_conv_refs(x, w, bias, dy):
    """The same for autograd.conv3x3; x (B, Ci, T, F), w (Co, Ci, 3, 3), dy (B, Co, T, F).  dx is the convolution of dy with the flipped,
    transposed kernel; dW[co, ci, kh, kw] = sum over positions of dy[.., t, f] x[.., t + kh - 1, f + kw - 1]."""
    import torch.nn.functional as F
    wt = w.flip(2, 3).transpose(0, 1).contiguous()
    xd, dyd = x.double(), dy.double()
    xp, xpa = F.pad(xd, (1, 1, 1, 1)), F.pad(xd.abs(), (1, 1, 1, 1))
    T, Fq = x.shape[2:]
    dw = torch.stack([torch.stack([torch.einsum('botf,bitf->oi', dyd, xp[:, :, kh:kh + T, kw:kw + Fq]) for kw in range(3)], -1) for kh in range(3)], -2)
    dwb = torch.stack([torch.stack([torch.einsum('botf,bitf->oi', dyd.abs(), xpa[:, :, kh:kh + T, kw:kw + Fq]) for kw in range(3)], -1) for kh in range(3)], -2)
    return {'y': conv_ref(x, w, bias), 'dx': conv_ref(dy, wt), 'dw': (to_f32(dw), dwb),
            'db': (to_f32(dyd.sum((0, 2, 3))), dyd.abs().sum((0, 2, 3)))}


# amtx_matmul_f32: the shapes of tests/test_gpu_poison.py (K = 4, 8: most slices of a split contraction are empty; (8, 12, 20000): the
# split contraction proper).  A 20000-term contraction leaves the fractional families no room (20000 * 3 * 2^7 = 2^22.9)
MATMUL_SHAPES = [(1, 4, 4), (37, 88, 256), (4999, 132, 36), (130, 1024, 176), (8, 12, 20000), (300, 36, 8), (132, 4, 3648), (260, 516, 4)]
MATMUL_FRAC_SHAPES = [s for s in MATMUL_SHAPES if s != (8, 12, 20000)]
MATMUL_CASES = [(s, 'int') for s in MATMUL_SHAPES] + [(s, fam) for s in MATMUL_FRAC_SHAPES for fam in ('frac_a', 'frac_b')]


def matmul_inputs(m, n, k, family):
    """(a (m, k), b (n, k), bias, grid step); family: 'int' | 'frac_a' | 'frac_b'."""
    g = gen(m, n, k, FAMILIES.index(family))
    a = fractional((m, k), INTS_A, g, TRAIN_S) if family == 'frac_a' else integers((m, k), INTS_A, g)
    b = fractional((n, k), INTS_W, g, TRAIN_S) if family == 'frac_b' else integers((n, k), INTS_W, g)
    return a, b, torch.randint(-8, 9, (n,), generator=g).float(), (1.0 if family == 'int' else 2.0 ** -TRAIN_S)
