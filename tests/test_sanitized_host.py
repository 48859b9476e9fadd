"""SURVEY section 5 / VERDICT r02 item 8: the HOST halves of the native library (weight packing, amtx_of_model_finalize, plan / basis
builders, C-ABI argument checks: hundreds of lines of index arithmetic) under AddressSanitizer + UndefinedBehaviorSanitizer, on the CPU
build only (the GPU pool refuses GPU ASan).  tests/san/build_san.py compiles them host-only with the sanitizers and links a host-memory
shim for the HIP runtime; tests/san/driver.py drives them in a child process that has clang's ASan runtime preloaded.  A report from
either sanitizer aborts the child."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'san'))


@pytest.fixture(scope='module')
def driver_run(tmp_path_factory):
    """One run of tests/san/driver.py under the sanitizers; it also writes the engine's decision table and upload hashes."""
    import build_san
    if not os.path.exists(build_san.HIPCC):
        pytest.skip('no hipcc: the sanitizer build needs the ROCm clang')
    lib = build_san.build()
    table = str(tmp_path_factory.mktemp('san') / 'of_conv_plan.json')
    env = dict(os.environ, LD_PRELOAD=build_san.asan_runtime(), ASAN_OPTIONS='detect_leaks=0:abort_on_error=1:halt_on_error=1',
               UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    for switch in ('AMTX_NO_CONVG_MC2', 'AMTX_NO_CONV_FUSE', 'AMTX_X3_NO_SPLIT', 'AMTX_NO_CONVX12M', 'AMTX_OF_ROWMAJOR_A3', 'AMTX_OF_NO_ROLL_EPILOGUE'):
        env.pop(switch, None)                 # the driver sets the create-time switches itself, one at a time
    p = subprocess.run([sys.executable, os.path.join(ROOT, 'tests', 'san', 'driver.py'), lib, table], env=env, capture_output=True, text=True, timeout=900)
    return p, table


def test_host_halves_of_the_library_are_clean_under_asan_and_ubsan(driver_run):
    p, _ = driver_run
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    assert 'no report' in p.stdout
    assert 'runtime error' not in p.stderr and 'AddressSanitizer' not in p.stderr, p.stderr[-6000:]


def test_engine_decisions_and_packed_weights_are_those_of_the_recorded_table(driver_run):
    """tests/golden/of_conv_plan.json was written by this driver on the commit BEFORE the engine's convolution path moved into one
    ConvPlan (ofmodel.hip): per model (model_complexity 2 .. 5 x 1, 2, 3, 6, 8, 9 input channels x bf16 / x3 / f16 x offset head x each
    create-time A/B switch alone or none; thinned at model_complexity 4 and 5, see the driver) what amtx_of_fuses_db_scale,
    amtx_of_takes_feats16, amtx_of_conv_stack_fused and amtx_of_workspace_bytes answer at five batch shapes and what
    amtx_of_model_finalize_device answers without tensors (its support check, or the first missing tensor); and for the driver's thirteen
    engine configurations the FNV-1a hash of every byte amtx_of_model_finalize uploads, in upload order.  Every row has to come back."""
    p, table = driver_run
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-6000:])
    with open(table) as f:
        got = json.load(f)
    with open(os.path.join(ROOT, 'tests', 'golden', 'of_conv_plan.json')) as f:
        want = json.load(f)
    assert got['plan_columns'] == want['plan_columns'] and got['upload_hash_columns'] == want['upload_hash_columns']
    assert len(want['plan_rows']) == 475 and len(want['upload_hashes']) == 13
    for key in ('plan_rows', 'upload_hashes'):
        assert len(got[key]) == len(want[key])
        wrong = [(g, w) for g, w in zip(got[key], want[key]) if g != w]
        assert not wrong, (key, len(wrong), wrong[:5])


def test_kernel_launches_are_those_of_the_recorded_trace():
    """tests/golden/launch_trace.json was recorded by tests/san/launch_trace.py on the commit BEFORE the GEMM launcher's routing became one
    function (gemm.hip: gemm_validate, gemm_route) and the doubled switches of conv.hip and convg.hip one accessor each.  With the shim
    recording launches (kernel name, grid, block, dynamic LDS bytes) instead of refusing them, once per A/B switch of those three files in
    a child process of its own: the return code, error text and launch of amtx_linear_fwd / amtx_linear_fwd_split over
    M {1, 255, 256, 1023, 1024, 4096} x N {4, 88, 128, 256, 512, 1024, 2048} x K {8, 64, 128, 176, 192, 512, 1024, 1088, 3648} x
    lda {K, K + 8} x (A type x C type x weight planes | two-plane A x C type), and every launch of amtx_of_forward, _power and _feats16 for
    the driver's thirteen engine configurations at (batch, frames) (2, 9), (3, 17), (130, 47), (43, 140), all outputs and rolls only, plus
    the bf16 model_complexity 2 configuration at (1024, 625), rolls only.  Every row and every sequence has to come back."""
    import build_san
    import launch_trace
    if not os.path.exists(build_san.HIPCC):
        pytest.skip('no hipcc: the sanitizer build needs the ROCm clang')
    env = dict(os.environ, LD_PRELOAD=build_san.asan_runtime(), ASAN_OPTIONS='detect_leaks=0:abort_on_error=1:halt_on_error=1',
               UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    got = launch_trace.record(build_san.build(), env)
    with open(os.path.join(ROOT, 'tests', 'golden', 'launch_trace.json')) as f:
        want = launch_trace.expand(json.load(f))
    assert tuple(want) == launch_trace.SWITCHES == tuple(got)
    for switch in launch_trace.SWITCHES:
        g, w = got[switch], want[switch]
        assert len(w['gemm']) == 15876 and len(w['engine']) == 170
        assert len(g['gemm']) == len(w['gemm']) and list(g['engine']) == list(w['engine'])
        wrong = [(i, a, b) for i, (a, b) in enumerate(zip(g['gemm'], w['gemm'])) if a != b]
        assert not wrong, (switch, 'gemm rows (index, got, want)', len(wrong), wrong[:5])
        wrong = [(k, g['engine'][k], b) for k, b in w['engine'].items() if g['engine'][k] != b]
        assert not wrong, (switch, 'engine sequences (name, got, want)', len(wrong), wrong[:2])
