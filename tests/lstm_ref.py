"""A plain float64 reference of the BiLSTM training recurrences of csrc/lstm.hip, the cases the tests run and their tolerances.

Host only: imports nothing but torch, calls no kernel.  tests/test_lstm_ref.py pins it to torch.nn.LSTM in float64 and proves that the
tolerances below can see a lost bf16 plane and a lost k-step; tests/test_gpu_bilstm_train.py holds the kernels to it.

Layouts are the kernels' (include/amtx.h), one LSTM at a time (the tests loop over the [groups] axis):
    xproj [B][T][2][4H]   W_ih x + b of both directions, gate order i, f, g, o
    whh_f, whh_b [4H][H]  recurrent weights of direction 0 (t = 0 .. T-1) and direction 1 (t = T-1 .. 0)
    out   [B][T][2H]      h of direction 0, then of direction 1
    save  [B][T][2][5][H] i, f, g, o AFTER their activation, then the cell state c
    dout  [B][T][2H]      dL/d(out);   dxproj [B][T][2][4H] = dL/d(xproj)

A mutation is (kind, arg), applied to ONE mat-vec (the forward's h W_hh^T or the backward's dgates W_hh) at every step of both directions:
    ('bf16', 'w')    W_hh rounded to bf16                      (a lost lo-plane of the weights)
    ('bf16', 'v')    the vector operand (h, dgates) rounded    (a lost lo-plane of the activations)
    ('drop', ks)     the 32 consecutive k indices 32 ks .. 32 ks + 31 left out of the sum (one MFMA k-step); k runs over the H hidden units
                     in the forward and over the 4H gate rows in the backward
"""
import torch

# ------------------------------------------------------------------------------------------------------------------------------
# Tolerances of tests/test_gpu_bilstm_train.py.
#   out:    max |out - ref|                                            <  TOL_OUT
#   save:   max |save[.., k, :] - ref| for each of i, f, g, o, c       <  TOL_SAVE * max(1, max |c_ref|)
#   dxproj: max |dxproj - ref|                                         <  TOL_DX * max |dxproj_ref|
# Each constant is 4 x the largest error measured on an MI355X over the eight CASES (headroom for other seeds and compilers), and sits
# under a cap that does not come from the kernels: TOL_OUT <= 3e-5 (what test_bilstm* hold the inference recurrences to), TOL_SAVE <= 3e-5,
# TOL_DX <= 3.2e-5 (a tenth of what losing one bf16 plane of the backward mat-vec moves dxproj by; tests/test_lstm_ref.py asserts the
# factor 10 for every single-plane loss and a factor 100 for every dropped k-step).
#
# Largest measured error per hidden size (two planes; `alone` = the backward kernel fed the reference's save, rounded to fp32):
#   hidden |   out   | save / max(1, max |c|) | dxproj / max, on the kernel's save | dxproj / max, alone
#     128  | 4.26e-6 |        2.30e-6         |              2.75e-6               |      1.62e-6
#     256  | 3.32e-6 |        2.14e-6         |              2.51e-6               |      1.33e-6
#     384  | 5.51e-6 |        2.52e-6         |              3.39e-6               |      1.51e-6
#     512  | 6.33e-6 |        2.67e-6         |              3.30e-6               |      1.67e-6
# (out: the saturated case (5, 19, 1, 6) at every size, 3.7e-6 at most without it; T = 1 stays under 2e-7: one step of fast exp / rcp.)
# For comparison, float64 on the CPU: the same recurrence in fp32 moves out by 1.6e-7, W_hh as hi + lo bf16 planes by 1.7e-6.
TOL_OUT = 2.6e-5         # 4 x 6.33e-6
TOL_SAVE = 1.1e-5        # 4 x 2.67e-6
TOL_DX = 1.4e-5          # 4 x 3.39e-6
CAP_OUT, CAP_SAVE, CAP_DX = 3e-5, 3e-5, 3.2e-5

HIDDEN = (128, 256, 384, 512)
# (B, T, groups, xproj scale): what each reaches is in the docstring of tests/test_gpu_bilstm_train.py
CASES = ((1, 1, 1, 1), (1, 2, 1, 1), (3, 5, 2, 1), (4, 19, 1, 1), (5, 19, 2, 1), (17, 7, 1, 1), (3, 96, 1, 1), (5, 19, 1, 6))


def make_case(H, B, T, G=1, scale=1):
    """Seeded fp32 inputs of G LSTMs: xproj [G][B][T][2][4H] ~ N(0, 1) * scale, whh_f / whh_b [G][4H][H] ~ U(+-0.15) at H = 128 and
    U(+-0.1) otherwise, dout [G][B][T][2H] ~ N(0, 1)."""
    g = torch.Generator().manual_seed(((H * 131 + B) * 131 + T) * 131 + G * 7 + scale)
    a = 0.15 if H == 128 else 0.1
    xproj = torch.randn(G, B, T, 2, 4 * H, generator=g) * float(scale)
    whh_f = (torch.rand(G, 4 * H, H, generator=g) * 2 - 1) * a
    whh_b = (torch.rand(G, 4 * H, H, generator=g) * 2 - 1) * a
    dout = torch.randn(G, B, T, 2 * H, generator=g)
    return {'xproj': xproj, 'whh_f': whh_f, 'whh_b': whh_b, 'dout': dout}


def _bf16(x):
    return x.to(torch.bfloat16).to(torch.float64)


def _matvec(v, w, mutate):
    """v [B][K] times w [K][N] in float64, with the mutation (module docstring) applied."""
    if mutate is not None:
        kind, arg = mutate
        if kind == 'bf16':
            assert arg in ('w', 'v')
            if arg == 'w':
                w = _bf16(w)
            else:
                v = _bf16(v)
        elif kind == 'drop':
            assert 0 <= 32 * arg and 32 * arg + 32 <= v.shape[1]
            keep = torch.ones(v.shape[1], dtype=torch.float64)
            keep[32 * arg:32 * arg + 32] = 0
            v = v * keep
        else:
            raise ValueError(mutate)
    return v @ w


def forward(xproj, whh_f, whh_b, mutate=None):
    """-> out [B][T][2H], save [B][T][2][5][H], float64."""
    B, T = xproj.shape[:2]
    H = whh_f.shape[1]
    assert xproj.shape == (B, T, 2, 4 * H) and whh_f.shape == whh_b.shape == (4 * H, H)
    x = xproj.double()
    out = torch.zeros(B, T, 2 * H, dtype=torch.float64)
    save = torch.zeros(B, T, 2, 5, H, dtype=torch.float64)
    for d, whh in enumerate((whh_f.double(), whh_b.double())):
        h = torch.zeros(B, H, dtype=torch.float64)
        c = torch.zeros(B, H, dtype=torch.float64)
        wt = whh.t().contiguous()                                  # [H][4H]: k = hidden unit
        for s in range(T):
            t = s if d == 0 else T - 1 - s
            gates = x[:, t, d] + _matvec(h, wt, mutate)
            i = torch.sigmoid(gates[:, 0 * H:1 * H])
            f = torch.sigmoid(gates[:, 1 * H:2 * H])
            g = torch.tanh(gates[:, 2 * H:3 * H])
            o = torch.sigmoid(gates[:, 3 * H:4 * H])
            c = f * c + i * g
            h = o * torch.tanh(c)
            out[:, t, d * H:(d + 1) * H] = h
            for k, v in enumerate((i, f, g, o, c)):
                save[:, t, d, k] = v
    return out, save


def backward(save, whh_f, whh_b, dout, mutate=None):
    """-> dxproj [B][T][2][4H], float64: the steps of each direction walked against their forward order,
        dh = dout_t + dgates_next W_hh;  do = dh tanh(c) o (1 - o);  dc = dc_next f_next + dh o (1 - tanh(c)^2)
        di = dc g i (1 - i);  dg = dc i (1 - g^2);  df = dc c_prev f (1 - f)
    (`next` = the step after this one in forward order, c_prev = the cell state before it, zero at the first step)."""
    B, T = save.shape[:2]
    H = whh_f.shape[1]
    assert save.shape == (B, T, 2, 5, H) and dout.shape == (B, T, 2 * H)
    sv, dy = save.double(), dout.double()
    dx = torch.zeros(B, T, 2, 4 * H, dtype=torch.float64)
    for d, whh in enumerate((whh_f.double(), whh_b.double())):
        frames = list(range(T)) if d == 0 else list(range(T - 1, -1, -1))       # forward order of this direction
        dh_rec = torch.zeros(B, H, dtype=torch.float64)
        dc_rec = torch.zeros(B, H, dtype=torch.float64)
        for s in range(T - 1, -1, -1):
            t = frames[s]
            i, f, g, o, c = (sv[:, t, d, k] for k in range(5))
            c_prev = sv[:, frames[s - 1], d, 4] if s > 0 else torch.zeros(B, H, dtype=torch.float64)
            dh = dy[:, t, d * H:(d + 1) * H] + dh_rec
            tc = torch.tanh(c)
            d_o = dh * tc * o * (1 - o)
            dc = dc_rec + dh * o * (1 - tc * tc)
            d_i = dc * g * i * (1 - i)
            d_g = dc * i * (1 - g * g)
            d_f = dc * c_prev * f * (1 - f)
            dc_rec = dc * f
            dgates = torch.cat([d_i, d_f, d_g, d_o], dim=1)        # [B][4H]: k = gate row
            dx[:, t, d] = dgates
            dh_rec = _matvec(dgates, whh, mutate)
    return dx


_REFS = {}


def reference(H, B, T, G=1, scale=1):
    """The case's inputs and its float64 results, every group: computed once per process, shared (do not write to it)."""
    key = (H, B, T, G, scale)
    if key not in _REFS:
        case = make_case(H, B, T, G, scale)
        outs, saves, dxs = [], [], []
        for g in range(G):
            out, save = forward(case['xproj'][g], case['whh_f'][g], case['whh_b'][g])
            outs.append(out)
            saves.append(save)
            dxs.append(backward(save, case['whh_f'][g], case['whh_b'][g], case['dout'][g]))
        case.update(out=torch.stack(outs), save=torch.stack(saves), dxproj=torch.stack(dxs))
        _REFS[key] = case
    return _REFS[key]
