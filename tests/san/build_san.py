"""TEST INFRASTRUCTURE: AddressSanitizer + UBSan build of the HOST halves of amt_tools_amd/csrc (weight packers, amtx_of_model_finalize,
spectrogram / CQT plan builders, the C-ABI argument checks), CPU only: `hipcc --cuda-host-only -fsanitize=address,undefined`, linked
against tests/san/hip_host_shim.cpp instead of the HIP runtime.  Output: tests/san/_build/libamtx_san.so (git-ignored, never shipped).
SURVEY section 5 / VERDICT r02 item 8: sanitizers run on the CPU build only (the GPU pool refuses GPU ASan)."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from amt_tools_amd.build import F16_TWINS  # noqa: E402  (the files compiled a second time with -DAMTX_F16)
CSRC = os.path.join(ROOT, 'amt_tools_amd', 'csrc')
OUT = os.path.join(HERE, '_build')
LIB = os.path.join(OUT, 'libamtx_san.so')
HIPCC = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
# -fno-sanitize=function: a kernel launched through a variable (`auto kern = some_kernel<...>; hipLaunchKernelGGL(kern, ...)`) is a call through
# the kernel's HANDLE, a constant that is no function; the function-type check reads in front of it, and the optimizer then drops the whole
# launch -- the host code behind it would run as if the kernel had been launched, with neither the shim's "no device" nor a trace record
SAN = ['-fsanitize=address,undefined', '-fno-sanitize=function', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-g', '-O1']


def asan_runtime():
    return subprocess.check_output([_clangxx(), '-print-file-name=libclang_rt.asan-x86_64.so'], text=True).strip()


def _newest_source():
    files = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(('.hip', '.cpp', '.h'))]
    files += [os.path.join(ROOT, 'include', 'amtx.h'), os.path.join(HERE, 'hip_host_shim.cpp'), os.path.abspath(__file__)]
    return max(os.path.getmtime(f) for f in files)


def _clangxx():
    return os.path.join(os.path.dirname(os.path.realpath(HIPCC)), '..', 'lib', 'llvm', 'bin', 'clang++')


def _hip_object(path, obj, extra=(), verbose=False):
    """The one compile recipe: a HIP source's host half with the sanitizers."""
    cmd = [HIPCC, '--cuda-host-only', '-std=c++17', '-fPIC', '-Wno-unused-function', '-DAMTX_WITH_F16'] + SAN + list(extra) + ['-x', 'hip', '-c', path, '-o', obj]
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return obj


def _jobs():
    return [(f, False) for f in sorted(os.listdir(CSRC)) if f.endswith(('.hip', '.cpp'))] + [(f, True) for f in F16_TWINS]


def _object_of(job):
    return os.path.join(OUT, os.path.splitext(job[0])[0] + ('_f16.o' if job[1] else '.o'))


def objects(verbose=False):
    """Every host-only object of csrc, the shim and the empty fat binaries they reference: what the library and a stand-alone program link."""
    os.makedirs(OUT, exist_ok=True)

    def cc(job):
        src, f16 = job
        return _hip_object(os.path.join(CSRC, src), _object_of(job), ['-DAMTX_F16'] if f16 else [], verbose)
    with ThreadPoolExecutor(max_workers=4) as ex:
        objs = list(ex.map(cc, _jobs()))
    # the host-only objects reference one __hip_fatbin_<hash> symbol each (the device code they were not built with): define them empty
    und = subprocess.check_output(['nm', '-u'] + objs, text=True)
    fat = sorted({l.split()[-1] for l in und.splitlines() if '__hip_fatbin_' in l})
    stub = os.path.join(OUT, 'fatbin_stubs.c')
    with open(stub, 'w') as f:
        for name in fat:
            f.write(f'const char {name}[8] = {{0}};\n')
    shim = _hip_object(os.path.join(HERE, 'hip_host_shim.cpp'), os.path.join(OUT, 'hip_host_shim.o'), verbose=verbose)
    stubo = os.path.join(OUT, 'fatbin_stubs.o')
    subprocess.run(['gcc', '-fPIC', '-c', stub, '-o', stubo], check=True)
    return objs + [shim, stubo]


def build(verbose=False):
    if os.path.exists(LIB) and os.path.getmtime(LIB) > _newest_source():
        return LIB
    # -Bsymbolic: the library's own hipMalloc / hipLaunchKernel ... (the shim) win over any HIP runtime already in the process
    cmd = [_clangxx(), '-shared', '-fPIC', '-Wl,-Bsymbolic'] + SAN + ['-o', LIB] + objects(verbose)
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return LIB


def build_program(name, verbose=False):
    """tests/san/<name>.cpp with its own main, linked with the same objects into an executable: the sanitizer runtime is part of it."""
    build(verbose)                                      # brings the objects up to date
    src, exe = os.path.join(HERE, name + '.cpp'), os.path.join(OUT, name)
    if os.path.exists(exe) and os.path.getmtime(exe) > max(os.path.getmtime(LIB), os.path.getmtime(src)):
        return exe
    objs = [_object_of(j) for j in _jobs()] + [os.path.join(OUT, 'hip_host_shim.o'), os.path.join(OUT, 'fatbin_stubs.o')]      # as objects() left them
    cmd = [_clangxx()] + SAN + ['-o', exe, _hip_object(src, os.path.join(OUT, name + '.o'), verbose=verbose)] + objs
    if verbose:
        print(' '.join(cmd), flush=True)
    subprocess.run(cmd, check=True)
    return exe


if __name__ == '__main__':
    print(build(verbose=True))
    sys.exit(0)
