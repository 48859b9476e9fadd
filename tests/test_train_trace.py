"""The training step's dense launch decisions (train.hip: xgemm_route, colsum_route, xconv_route, xwgrad_route, ConvWs) against the trace
recorded before they became routes.  CPU only: tests/san/train_trace.cpp is a stand-alone program built from the sanitizer objects of
tests/san/build_san.py and the recording shim, so AddressSanitizer and UBSan are part of the executable."""
import json
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'san'))


def test_training_launches_are_those_of_the_recorded_trace():
    """tests/golden/train_trace.json was recorded by tests/san/train_trace.py on commit 9dee499, BEFORE train.hip took its launch decisions
    from routes: per case the return code, the error text, the entry point's workspace query and every launch (kernel name with its template
    arguments, grid, block, dynamic LDS bytes) of
      - amtx_matmul_f32 in all four orientations, with and without bias, at M 1 .. 5000 x N 4 .. 512 x K 4 .. 160000 (31, 32 and 33 k-steps, 188
        and 192 output tiles), C padded or not, with no workspace, the query's answer, 4 bytes less and 1 MiB, and its refusals;
      - amtx_linear_train_fwd and amtx_linear_bwd for every subset of (dx, dw, db) at seven sizes (the flat, the row-split and the direct column
        sum), a padded dy, workspaces that halve the row groups or refuse the flat route, and the refusals;
      - amtx_conv3x3_train_fwd and amtx_conv3x3_bwd for eleven channel pairs at five map sizes, every subset of (dx, dw, db), workspaces that
        are exact, 1 MiB, one weight area, absent or a byte short, and the refusals.
    Every row has to come back; a report of either sanitizer fails the program."""
    import build_san
    import train_trace
    if not os.path.exists(build_san.HIPCC):
        pytest.skip('no hipcc: the sanitizer build needs the ROCm clang')
    got = train_trace.record()
    with open(os.path.join(ROOT, 'tests', 'golden', 'train_trace.json')) as f:
        golden = json.load(f)
    cases = train_trace.cases()
    assert golden['cases_sha256'] == train_trace.cases_sha256() and golden['parent_commit'] == '9dee499' and len(cases) == 18381
    want = train_trace.expand(golden)
    assert len(got) == len(want) == len(cases)
    wrong = [(c, a, b) for c, a, b in zip(cases, got, want) if a != b]
    assert not wrong, ('rows (case, got, want)', len(wrong), wrong[:5])
