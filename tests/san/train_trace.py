"""TEST INFRASTRUCTURE: the launch trace of the training step's dense entry points (amt_tools_amd/csrc/train.hip).

tests/san/train_trace.cpp -- a stand-alone program linked with the sanitizer build of the host halves and the recording shim -- reads the case
list `cases()` makes and prints, per case, the return code, the error text, what the entry point's workspace query answers and every kernel
launch (name, grid, block, dynamic LDS bytes).  train.hip reads no environment switch: one run.  tests/golden/train_trace.json is
`compact(record())` of the commit before train.hip's launch decisions became routes (`python tests/san/train_trace.py OUT.json COMMIT` writes
it, COMMIT being the commit recorded); tests/test_train_trace.py requires `expand` of it back from the present code.  The compact form is
tests/san/frontend_trace.py's, with the one run ''."""
import hashlib
import itertools
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import frontend_trace  # noqa: E402

MIB = 1 << 20          # what autograd._workspace allocates at least
SUBSETS = range(1, 8)  # every non-empty subset of (dx, dw, db) as 1 dx + 2 dw + 4 db

MATMUL_M = (1, 37, 128, 129, 5000)
MATMUL_N = (4, 32, 36, 64, 68, 88, 512)
MATMUL_K = (4, 32, 1020, 1024, 1028, 5000, 160000)         # 32-deep steps: 1, 1, 32, 32, 33 (splits start at 32), 157, 5000
# (m, n, k) beside the product of the three lists: 188 and 192 output tiles (splits stop at 192), the three tile widths at a short contraction
# and a split contraction of few tiles (what tests/test_gpu_train.py launches), a contraction that is no multiple of 4, 31 and 32 steps (the
# longest contraction in one piece, the shortest in two)
MATMUL_MORE = ((6016, 512, 1024), (6144, 512, 1024), (6016, 512, 5000), (6144, 512, 5000), (37, 32, 256), (37, 64, 256), (37, 88, 256), (88, 512, 5000),
               (37, 32, 6), (1, 4, 992), (1, 4, 996), (128, 64, 992))
MATMUL_WS = ('null', 'exact', 'exact-4', '=%d' % MIB)
LINEAR_SIZES = ((1, 4, 4), (37, 88, 256), (5000, 88, 512), (1024, 64, 176), (1023, 64, 176), (511, 64, 176), (625, 512, 3648))
CONV_CHANNELS = ((1, 32), (3, 32), (6, 32), (16, 16), (32, 32), (32, 64), (64, 32), (64, 64), (48, 96), (96, 96), (128, 128))
CONV_SHAPES = ((1, 1, 2), (14, 7, 13), (34, 17, 10), (192, 64, 229), (5000, 625, 229))           # (rows, frames per clip, bins)


def conv_ws_w(c_in, c_out):
    """Bytes of one of the two weight areas at the head of the convolution workspace."""
    return (9 * c_in * c_out * 4 + 255) // 256 * 256


def matmul_case(m, n, k, a_trans=0, b_trans=0, bias=1, ldc_pad=0, ws='exact', flaw='ok'):
    return 'matmul %d %d %d %d %d %d %d %s %s' % (m, n, k, a_trans, b_trans, bias, ldc_pad, ws, flaw)


def linear_fwd_case(m, n, k, bias=1, ldy_pad=0):
    return 'linear_fwd %d %d %d %d %d' % (m, n, k, bias, ldy_pad)


def linear_bwd_case(m, n, k, mask, lddy_pad=0, ws='exact', flaw='ok'):
    return 'linear_bwd %d %d %d %d %d %s %s' % (m, n, k, mask, lddy_pad, ws, flaw)


def conv_fwd_case(rows, t, f, c_in, c_out, bias=1, ws='exact'):
    return 'conv_fwd %d %d %d %d %d %d %s' % (rows, t, f, c_in, c_out, bias, ws)


def conv_bwd_case(rows, t, f, c_in, c_out, mask, ws='exact', flaw='ok'):
    return 'conv_bwd %d %d %d %d %d %d %s %s' % (rows, t, f, c_in, c_out, mask, ws, flaw)


def cases():
    """The one case list: lines of tests/san/train_trace.cpp's grammar."""
    lines = []
    for m, n, k in list(itertools.product(MATMUL_M, MATMUL_N, MATMUL_K)) + list(MATMUL_MORE):
        for at, bt, bias, pad, ws in itertools.product((0, 1), (0, 1), (0, 1), (0, 4), MATMUL_WS):
            lines.append(matmul_case(m, n, k, at, bt, bias, pad, ws))
    for flaw in ('null_a', 'null_c', 'odd_a', 'odd_b', 'lda', 'ldb'):
        lines.append(matmul_case(128, 64, 1024, flaw=flaw))
    lines += [matmul_case(0, 64, 1024), matmul_case(128, 0, 1024), matmul_case(128, 64, 0),
              matmul_case(4, 65536 * 128 + 4, 4, ws='null'), matmul_case(4, 65535 * 128, 4, ws='null')]        # 65537 (refused) and 65535 column tiles
    for m, n, k in LINEAR_SIZES:
        for bias, pad in itertools.product((0, 1), (0, 4)):
            lines.append(linear_fwd_case(m, n, k, bias, pad))
        for mask, ws in itertools.product(SUBSETS, ('exact', 'atleast=%d' % MIB, 'null')):
            lines.append(linear_bwd_case(m, n, k, mask, 0, ws))
    lines += [linear_bwd_case(1024, 64, 176, mask, 4) for mask in SUBSETS]                                   # a padded dy: never the flat column sum
    lines += [linear_bwd_case(5000, 88, 512, 4, ws='=%d' % b) for b in (19 * 88 * 4, 19 * 88 * 4 - 4, 4096, 704, 700, 0)]     # 19 row groups halved to 9, 2, 1
    lines += [linear_bwd_case(1024, 64, 176, 4, ws='=%d' % b) for b in (256 * 64 * 4, 256 * 64 * 4 - 4)]     # the flat route's partials fit / do not
    lines += [linear_bwd_case(37, 88, 256, 1, flaw='no_w'), linear_bwd_case(37, 88, 256, 2, flaw='no_x'), linear_bwd_case(37, 88, 256, 7, flaw='null_dy'),
              linear_bwd_case(0, 88, 256, 7), linear_bwd_case(37, 0, 256, 7), linear_bwd_case(37, 88, 0, 7), linear_bwd_case(37, 86, 256, 7), linear_bwd_case(37, 88, 254, 7)]
    for (c_in, c_out), (rows, t, f) in itertools.product(CONV_CHANNELS, CONV_SHAPES):
        for bias, ws in itertools.product((0, 1), ('exact', 'atleast=%d' % MIB, '=%d' % conv_ws_w(c_in, c_out), '=%d' % (conv_ws_w(c_in, c_out) - 1), 'null')):
            lines.append(conv_fwd_case(rows, t, f, c_in, c_out, bias, ws))
        for mask, ws in itertools.product(SUBSETS, ('exact', 'atleast=%d' % MIB, 'exact-1')):
            lines.append(conv_bwd_case(rows, t, f, c_in, c_out, mask, ws))
    # the strip kernel's weight image fits the forward's workspace exactly / is one byte short of fitting (the backward refuses any workspace
    # under its query's answer, which covers the image and the register-resident weight gradient's partials)
    for c_in, c_out, bn in ((32, 32, 32), (32, 64, 64), (64, 32, 32)):
        for short in (0, 1):
            lines.append(conv_fwd_case(34, 17, 10, c_in, c_out, 1, '=%d' % (2 * conv_ws_w(c_in, c_out) + 2 * bn * (18 * c_in + 16) - short)))
    lines += [conv_fwd_case(35, 17, 10, 32, 32), conv_bwd_case(35, 17, 10, 32, 32, 7), conv_fwd_case(0, 17, 10, 32, 32), conv_bwd_case(34, 0, 10, 32, 32, 7),
              conv_fwd_case(1 << 24, 64, 229, 32, 32), conv_bwd_case(1 << 24, 64, 229, 32, 32, 7),                 # 2^24 x 229 positions >= 2^31
              conv_fwd_case(34, 17, 10, 32, 30), conv_bwd_case(34, 17, 10, 32, 30, 7), conv_fwd_case(34, 17, 10, 1, 36), conv_fwd_case(34, 17, 10, 1, 32, ws='null'),
              conv_bwd_case(34, 17, 10, 32, 32, 1, flaw='no_w'), conv_bwd_case(34, 17, 10, 32, 32, 2, flaw='no_x'), conv_bwd_case(34, 17, 10, 32, 32, 7, ws='null')]
    return lines


def cases_sha256():
    return hashlib.sha256('\n'.join(cases()).encode()).hexdigest()


def record(exe=None):
    """[outcome per case]: [return code, error text, ['name<tab>numbers' ...]]; a report of either sanitizer ends the program with an error
    (the options of tests/test_sanitized_host.py)."""
    import build_san
    exe = exe or build_san.build_program('train_trace')
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, 'cases.txt')
        with open(path, 'w') as f:
            f.write('\n'.join(cases()) + '\n')
        env = dict(os.environ, ASAN_OPTIONS='detect_leaks=0:abort_on_error=1:halt_on_error=1', UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
        p = subprocess.run([exe, path], env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0 and 'runtime error' not in p.stderr and 'AddressSanitizer' not in p.stderr, (p.returncode, p.stdout[-2000:], p.stderr[-6000:])
    rows = frontend_trace.parse(p.stdout)
    assert len(rows) == len(cases()), len(rows)
    return rows


def compact(rows, parent_commit):
    return dict(frontend_trace.compact({'': rows}, cases_sha256()), parent_commit=parent_commit)


def expand(c):
    """The inverse of compact: [outcome per case], in the order of cases()."""
    return frontend_trace.expand(c)['']


if __name__ == '__main__':
    got = compact(record(), sys.argv[2])
    assert expand(got) == expand(json.loads(json.dumps(got)))
    frontend_trace.write(got, sys.argv[1])
