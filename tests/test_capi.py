"""CPU-side checks of the C ABI and its binding: the shared library loads and exports every symbol include/amtx.h declares, the ctypes
signatures read from the header equal the pinned table, and _lib.call / the pointer argument type behave.  No GPU here."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from amt_tools_amd import _lib

GOLDEN_ABI = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'abi_signatures.json')


def test_library_exports_every_declared_symbol():
    """Every declared function is exported, and the table parse_header reads from include/amtx.h equals tests/golden/abi_signatures.json
    exactly: row count, argument count and every letter (return type first; i int, l int64_t, z size_t, f float, d double, s const char*,
    p any other pointer; then whether the function ends in `void* stream`).  The golden was dumped from the hand-written ctypes table
    (_SIGNATURES in _lib.py) on the commit before the signatures were read from the header; a later header change shows up as a
    reviewed diff of that file."""
    L = _lib.lib()
    declared = _lib.declared_symbols()
    assert len(declared) >= 20
    for name in declared:
        assert hasattr(L, name), f'{name} declared in include/amtx.h but not exported'
    with open(GOLDEN_ABI) as f:
        golden = json.load(f)
    with open(_lib.HEADER_PATH) as f:
        parsed = {name: list(row) for name, row in _lib.parse_header(f.read()).items()}
    assert sorted(parsed) == sorted(golden) == declared
    for name in declared:
        assert parsed[name] == golden[name], (name, parsed[name], golden[name])
    assert L.amtx_version() >= 100


def _golden_name(header):
    """amtx.h -> abi_signatures.json, amtx_tracks.h -> abi_signatures_tracks.json."""
    return 'abi_signatures' + header[len('amtx'):-len('.h')] + '.json'


@pytest.mark.parametrize('header', _lib.HEADERS)
def test_every_header_is_bound_and_pinned_by_a_table_of_its_own(header):
    """Each header of _lib.HEADERS goes through the same parser, duplicate check and binding loop; its table equals its own golden file
    exactly (the notation of test_library_exports_every_declared_symbol; the file of amtx.h holds the table itself, every other file
    {header: table}), the golden directory holds one such file per header and no other, every declared name is exported and bound, and
    no name is declared in two headers."""
    assert _lib.HEADERS[0] == 'amtx.h' and len(set(_lib.HEADERS)) == len(_lib.HEADERS) and list(_lib.header_signatures()) == list(_lib.HEADERS)
    golden_dir = os.path.dirname(GOLDEN_ABI)
    assert sorted(f for f in os.listdir(golden_dir) if f.startswith('abi_signatures')) == sorted(_golden_name(h) for h in _lib.HEADERS)
    with open(os.path.join(golden_dir, _golden_name(header))) as f:
        golden = json.load(f)
    if header != 'amtx.h':
        assert list(golden) == [header]
        golden = golden[header]
    table = _lib.header_signatures()[header]
    assert {name: list(row) for name, row in table.items()} == golden and len(golden) >= 1
    assert (table is _lib.signatures()) == (header == 'amtx.h')
    L = _lib.lib()
    for name in golden:
        assert hasattr(L, name) and name in _lib._funcs, name
        assert [h for h in _lib.HEADERS if name in _lib.header_signatures()[h]] == [header], name
    with pytest.raises(_lib.AmtxError, match='amtx.h, amtx_tracks.h, amtx_pyramid.h, amtx_labels.h declare no function amtx_nothing'):
        _lib.call('amtx_nothing')


def test_a_name_declared_in_two_headers_is_refused(monkeypatch):
    monkeypatch.setattr(_lib, 'HEADERS', ('amtx.h', 'amtx_tracks.h', 'amtx_tracks.h'))
    monkeypatch.setattr(_lib, '_signatures', None)
    with pytest.raises(_lib.AmtxError, match='is declared in amtx_tracks.h and in another header'):
        _lib.header_signatures()


def test_parse_header_on_synthetic_text():
    table = _lib.parse_header("""
        #include <stdint.h>
        typedef struct amtx_thing amtx_thing;
        const char* amtx_name(void);   /* a void parameter list */
        int64_t amtx_run(const amtx_thing* thing, /* where */ const float* x /*[n]*/,
                         size_t n,      // how many
                         double a, float b, int32_t* out,
                         void* stream);
        int amtx_thing_create(amtx_thing** thing, const char* name, int flags);
    """)
    assert table == {'amtx_name': ('s', False), 'amtx_run': ('lppzdfpp', True), 'amtx_thing_create': ('ipsi', False)}
    for bad in ('int amtx_bad(long double x);', 'int amtx_bad(const float* x, void* stream, int n);', 'int amtx_bad(void (*fn)(int), int n);',
                'int amtx_bad(const void* stream);', 'struct amtx_s* amtx_bad(void);', 'int amtx_bad(int n)\nint amtx_worse(void);'):
        with pytest.raises(_lib.AmtxError, match='amtx_bad'):
            _lib.parse_header(bad)


def test_pointer_arguments():
    """A host-only packer gives the same bytes whichever accepted form carries its pointers; text and floats are no pointers."""
    n, k, planes = 7, 5, 2
    w = np.random.default_rng(0).standard_normal((n, k)).astype(np.float32)
    elems = _lib.call('amtx_linear_packed_elems', n, k, planes)
    forms = {'numpy': lambda a: a, 'ptr': _lib.ptr, 'c_void_p': lambda a: C.c_void_p(a.ctypes.data), 'address': lambda a: a.ctypes.data}
    packed = {}
    for form, conv in forms.items():
        out = np.full(elems, 0x5A5A, dtype=np.uint16)
        assert _lib.call('amtx_linear_pack', conv(w), n, k, planes, conv(out)) == 0
        packed[form] = out.tobytes()
    assert len(set(packed.values())) == 1 and packed['numpy'] != np.full(elems, 0x5A5A, dtype=np.uint16).tobytes()
    out = np.zeros(elems, dtype=np.uint16)
    for bad in ('text', 1.5):
        with pytest.raises(C.ArgumentError):
            _lib.call('amtx_linear_pack', bad, n, k, planes, out)
        with pytest.raises(C.ArgumentError):
            _lib.lib().amtx_linear_pack(_lib.ptr(w), n, k, planes, bad)
    w3 = np.random.default_rng(1).standard_normal((32, 32, 3, 3)).astype(np.float32)
    out3 = np.zeros(_lib.call('amtx_conv3x3_packed_elems', 32, 1), dtype=np.uint16)
    assert _lib.call('amtx_conv3x3_pack', w3, None, 32, 1, out3) == 0 and out3.any()             # None: the nullable scale


def test_call_reports_errors():
    h = C.c_void_p()
    with pytest.raises(_lib.AmtxError, match='amtx_of_model_create.*model_complexity'):
        _lib.call('amtx_of_model_create', C.byref(h), 229, 1, 6, 88, 1, 0)
    with pytest.raises(_lib.AmtxError, match='amtx_no_such'):
        _lib.call('amtx_no_such')
    for args in ((7, 5), (7, 5, 2, 1)):                                                          # one argument short, one too many
        with pytest.raises(TypeError, match='amtx_linear_packed_elems takes 3'):
            _lib.call('amtx_linear_packed_elems', *args)


def test_binding_imports_without_torch():
    """_lib.py loaded by file path, outside the package, in a process where torch cannot be imported: lib() and a host-only call work."""
    code = ('import sys, importlib.util\n'
            'sys.modules["torch"] = None\n'
            'spec = importlib.util.spec_from_file_location("amtx_lib_alone", sys.argv[1])\n'
            'm = importlib.util.module_from_spec(spec)\n'
            'spec.loader.exec_module(m)\n'
            'm.lib()\n'
            'assert m.call("amtx_version") >= 100 and m.call("amtx_last_error") is not None\n'
            'assert "torch" not in {k for k, v in sys.modules.items() if v is not None}\n'
            'print("ok", len(m.signatures()))\n')
    r = subprocess.run([sys.executable, '-c', code, _lib.__file__], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.startswith('ok'), r.stderr


def test_host_only_queries():
    L = _lib.lib()
    assert L.amtx_linear_packed_elems(88, 176, 1) == 128 * 192
    assert L.amtx_linear_packed_elems(512, 3648, 2) == 2 * 512 * 3648
    assert L.amtx_conv3x3_packed_elems(64, 1) == 9 * 4 * 512
    assert L.amtx_bilstm_packed_elems(2) == 2 * 2 * 512 * 128
    assert L.amtx_bilstm_h_packed_elems(256, 1) == 2 * 1024 * 256 and L.amtx_bilstm_h_packed_elems(128, 2) == L.amtx_bilstm_packed_elems(2)
    assert L.amtx_conv3x3g_packed_elems(48, 96, 1) == 6 * 14 * 512 and L.amtx_conv3x3g_packed_elems(32, 40, 1) == 0


def test_errors_are_reported_not_swallowed():
    L = _lib.lib()
    h = C.c_void_p()
    rc = L.amtx_of_model_create(C.byref(h), 229, 1, 6, 88, 1, 0)    # model_complexity 6: no kernels for its channel counts
    assert rc < 0 and b'model_complexity' in L.amtx_last_error()
    with pytest.raises(_lib.AmtxError):
        _lib.check(rc, 'amtx_of_model_create')
    assert os.path.exists(_lib.LIB_PATH)


def test_missing_extension_fails_loudly_without_a_cpu_fallback(monkeypatch):
    """No HIP extension -> the product path raises; nothing quietly computes on the CPU (oracle/ is never imported by the package)."""
    from amt_tools_amd.features import MelSpec
    monkeypatch.setattr(_lib, '_lib', None)
    monkeypatch.setattr(_lib, 'LIB_PATH', '/nonexistent/libamtx.so')
    with pytest.raises(_lib.AmtxError, match='no CPU fallback'):
        _lib.lib()
    with pytest.raises(Exception):          # AmtxError (no library) -- never a silently computed spectrogram
        MelSpec(sample_rate=22050).process_audio(np.zeros(4096, dtype=np.float32))
    assert not any(m == 'oracle' or m.startswith('oracle.') for m in sys.modules if 'amt_tools_amd' in str(getattr(sys.modules[m], '__file__', '')))
    import amt_tools_amd, pathlib
    src = ''.join(p.read_text() for p in pathlib.Path(amt_tools_amd.__file__).parent.glob('*.py'))
    assert 'import oracle' not in src and 'from oracle' not in src


# Arguments the convolution launchers refuse before anything is launched: (entry point, arguments after the pointers, return code, amtx_last_error).
# Dummy non-null host pointers; shape B 1, T 17, F 10 unless the case says otherwise.  conv3x3_fwd: (elem_type, planes, B, T, F, c_out, null input);
# conv3x3g_fwd: (elem_type, planes, B, T, F, c_in, c_out); conv1_fwd: (out_type, B, T, F, c_in, c_out).
CONV_REFUSALS = [
    ('amtx_conv3x3_fwd', (0, 1, 1, 17, 10, 48, False), -3, 'conv3x3: unsupported c_out=48 (supported: 32 and 64, with C_in = 32)'),
    ('amtx_conv3x3_fwd', (2, 1, 1, 17, 10, 32, False), -3, 'conv3x3: in/out element types must match (bf16/bf16 or f32/f32)'),
    ('amtx_conv3x3_fwd', (2, 2, 1, 17, 10, 32, False), -1, 'conv3x3: two-plane maps need plane strides'),
    ('amtx_conv3x3_fwd', (0, 1, 1, 17, 1, 32, False), -1, 'conv3x3: bad sizes'),
    ('amtx_conv3x3_fwd', (0, 1, 0, 17, 10, 32, False), -1, 'conv3x3: bad sizes'),
    ('amtx_conv3x3_fwd', (0, 3, 1, 17, 10, 32, False), -1, 'conv3x3: planes must be 1 or 2'),
    ('amtx_conv3x3_fwd', (0, 1, 1, 17, 10, 32, True), -1, 'conv3x3: null pointer'),
    ('amtx_conv3x3g_fwd', (0, 1, 1, 17, 10, 40, 32), -3, 'conv3x3 (general): unsupported channel counts 40 -> 32'),
    ('amtx_conv3x3g_fwd', (1, 1, 1, 17, 10, 48, 48), -3, 'conv3x3 (general): unsupported precision/type combination'),
    ('amtx_conv3x3g_fwd', (0, 2, 1, 17, 10, 64, 64), -3, 'conv3x3 (general): unsupported precision/type combination'),
    ('amtx_conv3x3g_fwd', (0, 1, 1, 17, 1, 48, 48), -1, 'conv3x3 (general): bad sizes'),
    ('amtx_conv1_fwd', (1, 1, 17, 10, 1, 12), -1, 'conv1: bad sizes'),
    ('amtx_conv1_fwd', (1, 1, 17, 10, 64, 64), -1, 'conv1: weights do not fit LDS'),
]


@pytest.mark.parametrize('entry,args,code,text', CONV_REFUSALS, ids=[f'{e[5:]}-{i}' for i, (e, *_) in enumerate(CONV_REFUSALS)])
def test_conv_launchers_refuse_with_the_recorded_code_and_text(entry, args, code, text):
    """Return code and amtx_last_error of the op-level convolution entry points for arguments their checks and routes refuse, as recorded
    before the launchers were split into checks -> route -> launch.  Nothing reaches a launch, so this needs no GPU."""
    L = _lib.lib()
    host = np.zeros(64, dtype=np.float32)
    p = _lib.ptr(host)
    if entry == 'amtx_conv3x3_fwd':
        elem, planes, b, t, f, c_out, null_in = args
        rc = L.amtx_conv3x3_fwd(None if null_in else p, elem, p, planes, p, p, b, t, f, c_out, None)
    elif entry == 'amtx_conv3x3g_fwd':
        elem, planes, b, t, f, c_in, c_out = args
        rc = L.amtx_conv3x3g_fwd(p, elem, p, planes, p, p, b, t, f, c_in, c_out, None)
    else:
        out_type, b, t, f, c_in, c_out = args
        rc = L.amtx_conv1_fwd(p, f * t, 0, f, 1, p, p, p, out_type, b, t, f, c_in, c_out, None)
    assert (rc, L.amtx_last_error().decode()) == (code, text)


def test_training_workspace_queries_answer_zero_splits_for_an_empty_problem():
    """xgemm_route refuses an empty problem before it counts tiles: amtx_matmul_workspace_bytes of a problem without rows or columns and a long
    contraction (32 k-steps or more) answers 0 -- it used to divide by the tile count -- and the queries built on it stay finite.  Host only."""
    L = _lib.lib()
    assert L.amtx_matmul_workspace_bytes(0, 64, 1024) == 0 and L.amtx_matmul_workspace_bytes(128, 0, 1024) == 0 and L.amtx_matmul_workspace_bytes(128, 64, 0) == 0
    assert L.amtx_linear_bwd_workspace_bytes(4096, 0, 64) == 256 and L.amtx_conv3x3_train_workspace_bytes(5000, 229, 0, 32) == 768 * 288 * 32 * 4 + 256
    assert L.amtx_matmul_workspace_bytes(1, 4, 996) == 32          # the smallest split problem still asks for its two partial tiles
