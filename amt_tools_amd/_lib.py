"""
ctypes binding of the amtx C ABI (the headers of HEADERS under include/ -> amt_tools_amd/csrc/libamtx.so).

Every header is read by parse_header, every function it declares is bound by lib() and reached through call(); header_signatures() holds
one table per header, and a name declared in two headers is an error.  tests/golden/ pins each header's table in a file of its own.

The product path has NO fallback: if the shared library is missing or a call fails, an exception is
raised.  Pointers handed to the library are raw device addresses (`tensor.data_ptr()`), the stream is
the current torch HIP stream's handle.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('AMTX_LIB_PATH') or os.path.join(_HERE, 'csrc', 'libamtx.so')      # AMTX_LIB_PATH: a debug / timing build of the same ABI
HEADER_PATH = os.path.join(os.path.dirname(_HERE), 'include', 'amtx.h')
# Every header of the library, bound the same way; a new header is appended here and gets a pinned table of its own under tests/golden/.
HEADERS = ('amtx.h', 'amtx_tracks.h', 'amtx_pyramid.h', 'amtx_labels.h', 'amtx_optim.h', 'amtx_noteclips.h', 'amtx_stitch.h', 'amtx_cliploss.h',
           'amtx_ofseq.h', 'amtx_thrgrid.h')
_PINNED_HEADERS = 4        # call()'s "declare no function" text lists these four in this order (pinned by tests/test_capi.py); later headers go in front

_lib = None


class AmtxError(RuntimeError):
    pass


ERR_UNSUPPORTED = -3       # AMTX_ERR_UNSUPPORTED (include/amtx.h)


class _Pointer(C.c_void_p):
    """The argument type of every pointer parameter but `const char*`: what c_void_p takes (None, a c_void_p, an integer address, byref(...),
    a ctypes array or pointer) plus anything with data_ptr() (a torch tensor, host or device) or .ctypes.data (a numpy array).  Text is no
    address: str and bytes, which c_void_p would pass as a pointer to their characters, are refused like every other type."""
    @classmethod
    def from_param(cls, obj):
        if hasattr(obj, 'data_ptr'):
            obj = obj.data_ptr()
        elif hasattr(obj, 'ctypes'):
            obj = obj.ctypes.data
        elif isinstance(obj, (str, bytes)):
            raise TypeError('a pointer argument, not text')
        return C.c_void_p.from_param(obj)


# One letter per C type: the notation of tests/golden/abi_signatures.json.
_CTYPES = {'i': C.c_int, 'l': C.c_int64, 'z': C.c_size_t, 'f': C.c_float, 'd': C.c_double, 's': C.c_char_p, 'p': _Pointer}
_SCALARS = {'int': 'i', 'int64_t': 'l', 'size_t': 'z', 'float': 'f', 'double': 'd'}
_POINTEES = {'void', 'float', 'double', 'int', 'int32_t', 'int64_t', 'uint16_t', 'uint8_t'}       # plus the handle structs the header typedefs
_PARAM = re.compile(r'(const )?(\w+) ?(\*{0,2}) ?(\w*)')


def parse_header(text):
    """{name: (letters, ends_in_stream)} for every function a header in the style of include/amtx.h declares: letters = the return type,
    then one letter per parameter (_CTYPES; 'p' = any pointer but `const char*`), ends_in_stream = the last parameter is `void* stream`.
    Between two ';' there is a handle typedef or such a declaration; anything else raises AmtxError -- nothing is skipped or guessed."""
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*(#.*|extern "C" \{|\})[ \t]*$', '', text, flags=re.M)      # preprocessor lines and the extern "C" bracket
    handles, table = set(), {}

    def letter(decl, param, is_return=False):
        """(letter, parameter name) of one `type name`."""
        m = _PARAM.fullmatch(param)
        if m:
            const, base, stars, name = m.groups()
            if not stars and not const and base in _SCALARS:
                return _SCALARS[base], name
            if stars == '*' and const and base == 'char':
                return 's', name
            if stars and not is_return and (base in _POINTEES or base in handles):
                return 'p', name
        raise AmtxError(f'cannot map "{param}" in the declaration "{decl}"')

    for decl in (' '.join(d.split()) for d in text.split(';')):
        m = re.fullmatch(r'typedef struct (\w+) \1', decl)
        if m:
            handles.add(m.group(1))
            continue
        m = re.fullmatch(r'(.*?) ?\b(amtx_\w+) ?\((.*)\)', decl)
        if not m:
            if decl:
                raise AmtxError(f'cannot read the declaration "{decl}"')
            continue
        ret, name, params = m.groups()
        if name in table:
            raise AmtxError(f'{name} is declared twice')
        params = [] if params.strip() == 'void' else [p.strip() for p in params.split(',')]
        letters, names = letter(decl, ret, is_return=True)[0], []
        for param in params:
            code, pname = letter(decl, param)
            letters += code
            names.append(pname)
        if 'stream' in names and (names.index('stream') != len(names) - 1 or params[-1].replace(' ', '') != 'void*stream'):
            raise AmtxError(f'`stream` must be the last parameter and a `void*` in the declaration "{decl}"')
        table[name] = (letters, 'stream' in names)
    return table


_signatures = None


def header_signatures():
    """{header: parse_header of it} for every header of HEADERS, read once per process.  A name declared in two headers raises."""
    global _signatures
    if _signatures is None:
        tables, seen = {}, set()
        for header in HEADERS:
            with open(os.path.join(os.path.dirname(HEADER_PATH), header)) as f:
                tables[header] = parse_header(f.read())
            twice = seen & set(tables[header])
            if twice:
                raise AmtxError(f'{sorted(twice)[0]} is declared in {header} and in another header')
            seen |= set(tables[header])
        _signatures = tables
    return _signatures


def signatures():
    """The table of include/amtx.h alone."""
    return header_signatures()['amtx.h']


def declared_symbols():
    """Every function name include/amtx.h declares."""
    return sorted(signatures())


_funcs = {}            # name -> (function, number of parameters, its return value goes through check, it ends in `void* stream`)


def lib():
    """Load libamtx.so (once) and give every function the headers of HEADERS declare its restype / argtypes.  Raises AmtxError when the HIP
    extension has not been built, when it lacks a declared function, or when a header holds a declaration parse_header cannot map."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise AmtxError(f'{LIB_PATH} is missing: build the HIP extension first '
                            f'(python -m amt_tools_amd.build, or __graft_entry__.build()). '
                            f'There is no CPU fallback for the product path.')
        try:
            handle = C.CDLL(LIB_PATH)
        except OSError as e:
            raise AmtxError(f'cannot load {LIB_PATH}: {e}') from e
        for table in header_signatures().values():
            for name, (letters, stream) in table.items():
                try:
                    fn = getattr(handle, name)
                except AttributeError as e:
                    raise AmtxError(f'{LIB_PATH} does not export {name}') from e
                fn.restype = _CTYPES[letters[0]]
                fn.argtypes = [_CTYPES[c] for c in letters[1:]]
                _funcs[name] = (fn, len(letters) - 1, letters[0] in 'il', stream)
        _lib = handle
    return _lib


def call(name, *args, device=None):
    """Call the library's function `name`; tensors and arrays are passed as they are (_Pointer).  With `device`, the call runs under
    torch.cuda.device(device), and a function whose last parameter is `void* stream` gets that device's current stream appended -- the
    caller passes one argument fewer.  Without `device` the arguments go through as given (host-only functions, an explicit stream).
    A signed integer return goes through check(); any other return value comes back as it is.  A wrong number of arguments is a TypeError
    before the library is entered (ctypes alone lets surplus arguments through)."""
    lib()
    try:
        fn, nargs, checked, stream = _funcs[name]
    except KeyError:
        searched = ", ".join(HEADERS[_PINNED_HEADERS:] + HEADERS[:_PINNED_HEADERS])
        raise AmtxError(f'{searched} declare no function {name}') from None
    fill_stream = stream and device is not None
    if len(args) + fill_stream != nargs:
        raise TypeError(f'{name} takes {nargs - fill_stream} arguments{" besides the stream" if fill_stream else ""} ({len(args)} given)')
    if device is None:
        rc = fn(*args)
    else:
        import torch
        with torch.cuda.device(device):
            rc = fn(*args, current_stream(device)) if stream else fn(*args)
    return check(rc, name) if checked else rc


def check(rc, what=''):
    if rc is None or rc < 0:
        msg = lib().amtx_last_error()
        raise AmtxError(f'{what} failed ({rc}): {msg.decode() if msg else "?"}')
    return rc


def ptr(t):
    """Device (or host) address of a torch tensor / numpy array, or None."""
    if t is None:
        return None
    if hasattr(t, 'data_ptr'):
        return C.c_void_p(t.data_ptr())
    return C.c_void_p(t.ctypes.data)


def current_stream(device=None):
    import torch
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


# ------------------------------------------------------------------------------------------------------------------------------
# kernel workspaces with guard bands (tests/test_gpu_guards.py)
# ------------------------------------------------------------------------------------------------------------------------------
GUARD_BYTES = 0        # > 0 (a multiple of 256): every workspace below gets this many pattern-filled bytes in front of and behind it
_GUARD_PATTERN = 0xA5
_GUARDED = {}          # data_ptr of a guarded workspace view -> (weak reference to its full allocation, guard bytes)


def alloc_workspace(nbytes, device):
    """uint8 tensor of `nbytes` for a kernel workspace.  With GUARD_BYTES set it is the middle of a larger allocation whose first and last
    GUARD_BYTES hold a pattern: several kernels issue masked stores to scratch lines and loads from clamped addresses, and a store that
    leaves its workspace must not go unnoticed (guards_intact)."""
    import torch
    nbytes = int(nbytes)
    g = int(GUARD_BYTES)
    if g <= 0:
        return torch.empty(nbytes, dtype=torch.uint8, device=device)
    assert g % 256 == 0
    full = torch.empty(nbytes + 2 * g, dtype=torch.uint8, device=device)
    full[:g] = _GUARD_PATTERN
    full[g + nbytes:] = _GUARD_PATTERN
    ws = full[g:g + nbytes]                        # a view: keeps `full` alive, data_ptr() is 256-byte aligned like the allocation
    import weakref
    for k in [k for k, (r, _) in _GUARDED.items() if r() is None]:
        del _GUARDED[k]
    _GUARDED[ws.data_ptr()] = (weakref.ref(full), g)
    return ws


def guards_intact(ws):
    """True when the bands around a workspace from alloc_workspace still hold the pattern.  Only tensors alloc_workspace itself handed out
    with guard bands are checked (they are recorded there); anything else -- an unguarded workspace, a plain view of some other buffer --
    has no bands and answers True."""
    rec = _GUARDED.get(ws.data_ptr())
    base = getattr(ws, '_base', None)
    if rec is None or base is None or rec[0]() is not base:
        return True
    g = rec[1]
    return bool((base[:g] == _GUARD_PATTERN).all().item()) and bool((base[g + ws.numel():] == _GUARD_PATTERN).all().item())
