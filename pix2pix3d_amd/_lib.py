"""ctypes binding of libp3d_hip.so (C ABI declared in include/p3d_hip.h).

The library is mandatory for CUDA/HIP tensors: ``lib()`` raises if it cannot be loaded, and no op
in this package has a GPU fallback.  torch is imported first so the HIP runtime the library binds
to (SONAME libamdhip64.so.7) is the one torch already mapped — streams and device pointers are
then shared between torch and the kernels.
"""
import ctypes
import os
import re
import threading

import torch  # noqa: F401  (must precede CDLL: see module docstring)

from . import build

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('P3D_LIB_PATH') or os.path.join(_PKG_DIR, 'libp3d_hip.so')      # (P3D_LIB_PATH: A/B runs of two builds on one box)

FAMILY = {'bias_act': 0, 'upfirdn2d': 1, 'filtered_lrelu': 2, 'render': 3, 'conv': 4, 'aux': 5}

_c_void_p = ctypes.c_void_p
_i32x4, _i64x4 = ctypes.c_int32 * 4, ctypes.c_int64 * 4
_i32x2, _i64x2 = ctypes.c_int32 * 2, ctypes.c_int64 * 2

_C_TYPES = {'int': ctypes.c_int32, 'int16_t': ctypes.c_int16, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'uint8_t': ctypes.c_uint8, 'uint32_t': ctypes.c_uint32,
            'uint64_t': ctypes.c_uint64, 'float': ctypes.c_float, 'double': ctypes.c_double}
_DECLARATOR = re.compile(r'(.*?)(\w+)\s*(?:\[\s*(\d*)\s*\])?', re.S)      # [type] name [[n]]
_INTEGER = re.compile(r'(-?(?:0[xX][0-9a-fA-F]+|\d+))(?:[uU](?:ll?|LL?)?|(?:ll?|LL?)[uU]?)?')      # a C integer literal and its suffix (u, l, ll)


def _integer(text):
    m = _INTEGER.fullmatch(text)
    if not m:
        raise ValueError(f'header: {text!r} is not an integer literal')
    return int(m.group(1), 0)


class Header:
    """What one of this project's C99 headers declares, as ctypes needs it: ``functions`` name -> (restype, argtypes), ``structs`` name ->
    ctypes.Structure class, ``constants`` name -> int (every integer ``#define P3D_*`` and every enumerator).  Every pointer and array
    parameter is a c_void_p (None, c_void_p, ctypes arrays, byref() and pointer() all convert to it); anything it cannot read is an error."""

    def __init__(self, text, base=None):
        self.types = dict(base.types if base else _C_TYPES)      # C name -> ctypes type; typedefs and structs join it (base: an #included header)
        self.functions, self.structs, self.constants = {}, {}, {}
        text = re.sub(r'/\*.*?\*/', ' ', text, flags=re.S)
        for name, value in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(P3D_\w+)[ \t]+\(?(-?\w+)\)?[ \t]*$', text, flags=re.M):
            self.constants[name] = _integer(value)
        text = re.sub(r'^[ \t]*#.*$|extern\s+"C"\s*\{', '', text, flags=re.M)
        text = re.sub(r'\benum\s*\w*\s*\{([^}]*)\}', self._enum, text)
        text = re.sub(r'\btypedef\s+struct\s*\w*\s*\{([^}]*)\}\s*(\w+)', self._struct, text)
        for statement in filter(None, map(str.strip, text.replace('}', ';').split(';'))):      # (the '}' left over closes extern "C")
            typedef = re.fullmatch(r'typedef\s+void\s*\*\s*(\w+)', statement)
            proto = re.fullmatch(r'(.*?)(\w+)\s*\((.*)\)', statement, flags=re.S)
            if typedef:
                self.types[typedef.group(1)] = ctypes.c_void_p
            elif proto:
                ret, name, params = proto.groups()
                argtypes = [] if params.strip() in ('', 'void') else [self._declare(name, p)[1] for p in params.split(',')]
                self.functions[name] = (self._ctype(name, ret, returned=True), argtypes)
            else:
                raise ValueError(f'header: cannot parse {" ".join(statement.split())!r}')

    def _enum(self, m):
        value = -1
        for item in filter(None, map(str.strip, m.group(1).split(','))):
            name, _, given = map(str.strip, item.partition('='))
            self.constants[name] = value = _integer(given) if given else value + 1
        return ''

    def _struct(self, m):
        name, fields = m.group(2), []
        for members in filter(None, map(str.strip, m.group(1).split(';'))):
            ctype = ''
            for member in members.split(','):                       # int32_t ci, co;
                field, t, ctype = self._declare(name, member, ctype, member=True)
                fields.append((field, t))
        self.structs[name] = self.types[name] = type(name, (ctypes.Structure,), {'_fields_': fields})
        return ''

    def _declare(self, symbol, text, ctype='', member=False):
        """(name, ctypes type, C type) of a parameter or struct member; ``ctype``: the type a member list began with."""
        m = _DECLARATOR.fullmatch(text.strip())
        own = m.group(1).strip() if m else ''
        if not (own or ctype) or (not own and ctype.endswith('*')):
            raise ValueError(f'header: {symbol}: cannot parse {text.strip()!r}')
        t = self._ctype(symbol, own or ctype)
        if m.group(3) is not None:
            t = t * int(m.group(3)) if member else ctypes.c_void_p      # an array parameter is a pointer
        return m.group(2), t, own or ctype

    def _ctype(self, symbol, ctype, returned=False):
        words = ' '.join(w for w in ctype.replace('*', ' * ').split() if w != 'const')
        if words.endswith('*'):
            return ctypes.c_char_p if returned and words == 'char *' else ctypes.c_void_p
        if words not in self.types:
            raise ValueError(f'header: {symbol}: unknown type {" ".join(ctype.split())!r}')
        return self.types[words]

    def bind(self, handle):
        """Set restype / argtypes of every declared function on a loaded library (AttributeError if one is not exported: a stale build)."""
        for name, signature in self.functions.items():
            fn = getattr(handle, name)
            fn.restype, fn.argtypes = signature


def read_header(path, base=None):
    with open(path) as f:
        return Header(f.read(), base)


# include/p3d_hip.h is the only description of the ABI: every signature, struct and constant on the Python side is read from it, here,
# and _load binds every function it declares (a library exports nothing that its header does not declare: tests/test_side_libraries.py).
HEADER = read_header(os.path.join(os.path.dirname(_PKG_DIR), 'include', 'p3d_hip.h'))
globals().update(HEADER.constants)      # _lib.P3D_OK, _lib.P3D_F32_BF16X3, _lib.P3D_FRAME_MAX_JOBS, ...: under their C names
globals().update(HEADER.structs)        # _lib.p3d_render_desc, _lib.p3d_demod_job, _lib.p3d_fc_job, _lib.p3d_frame_job
DTYPE_CODE = {torch.float32: HEADER.constants['P3D_F32'], torch.float16: HEADER.constants['P3D_F16'], torch.float64: HEADER.constants['P3D_F64']}

_lib = None
_load_error = None
kernel_events = {}      # name -> list of (start, end) torch.cuda.Event pairs; filled only while a key exists (bench.py)


def _load():
    global _lib, _load_error
    if _lib is not None or _load_error is not None:
        return
    try:
        handle = ctypes.CDLL(LIB_PATH)
        HEADER.bind(handle)
        _lib = handle
    except (OSError, AttributeError) as e:      # missing file, unresolved HIP runtime, stale build
        _load_error = e


def available():
    _load()
    return _lib is not None


_tls = threading.local()       # .device: ordinal of the tensor the pending call's stream was taken from (set by stream_of)


class _Guarded:
    """The library handle with a device guard around every entry point: a kernel must be enqueued with ITS tensors' device
    current (the reference plugins wrap each op in ``OptionalCUDAGuard(device_of(x))``, bias_act.cpp:57), not whatever device the
    caller last selected.  ``stream_of(t)`` — evaluated while the call's arguments are built — notes t's device; the call then
    switches to it for its duration when it is not the current one."""

    def __init__(self, handle):
        self._handle, self._fns = handle, {}

    def __getattr__(self, name):
        fn = self._fns.get(name)
        if fn is None:
            raw = getattr(self._handle, name)

            def fn(*args, _raw=raw):
                dev, _tls.device = getattr(_tls, 'device', None), None
                if dev is None or dev == torch.cuda.current_device():
                    return _raw(*args)
                with torch.cuda.device(dev):
                    return _raw(*args)
            self._fns[name] = fn
        return fn


_guarded = None


def lib():
    """Return the loaded library (device-guarded) or raise: there is no fallback for device tensors."""
    global _guarded
    _load()
    if _lib is None:
        raise RuntimeError(
            f'pix2pix3d_amd: the gfx950 kernel library {LIB_PATH} could not be loaded ({_load_error}). '
            'Build it with `python -m pix2pix3d_amd.build` (or __graft_entry__.build()); '
            'CUDA/HIP tensors have no fallback path in this package.')
    if _guarded is None:
        _guarded = _Guarded(_lib)
    return _guarded


def check(code, what):
    if code != HEADER.constants['P3D_OK']:
        msg = lib().p3d_last_error().decode('utf-8', 'replace')
        raise RuntimeError(f'{what}: libp3d_hip error {code}: {msg}')


class SideLibrary:
    """A kernel library beside libp3d_hip.so (a row of ``build.SIDE_LIBRARIES``): ``header`` is its own header, read on top of the product's (which it
    includes for p3d_stream_t and the status codes), and the only description of the library's ABI — every module that calls the library reads its
    constants from ``header`` and calls through ``lib()``, which binds all the header declares; ``lib()`` is the loaded library (device-guarded) or
    RuntimeError — device tensors have no fallback."""

    def __init__(self, name):
        paths = build.side_paths(name)
        self.name, self.path, self.header = name, paths.lib, read_header(paths.header, base=HEADER)
        self._raw = self._guarded = None

    def lib(self):
        if self._guarded is None:
            lib()                                                   # maps the HIP runtime torch uses first
            try:
                h = ctypes.CDLL(self.path)
            except OSError as e:
                raise RuntimeError(f'pix2pix3d_amd: {self.path} could not be loaded ({e}); build it with `python -m pix2pix3d_amd.build`')
            for service in ('p3d_last_error', 'p3d_launch_count'):      # the library's own copy of the library services
                fn = getattr(h, service)
                fn.restype, fn.argtypes = HEADER.functions[service]
            self.header.bind(h)
            self._raw, self._guarded = h, _Guarded(h)
        return self._guarded

    def launch_count(self):
        """Kernel launches of this library so far (its own counter: the product's ``launch_count`` does not see them)."""
        self.lib()
        return int(self._raw.p3d_launch_count())

    def check(self, code, what):
        if code != HEADER.constants['P3D_OK']:
            raise RuntimeError(f'{what}: libp3d_{self.name} error {code}: {self.lib().p3d_last_error().decode("utf-8", "replace")}')


def stream_of(t):
    """Current stream of t's device (what the reference plugins launch on) — and tell the device guard which device that is."""
    _tls.device = t.device.index
    return _c_void_p(torch.cuda.current_stream(t.device).cuda_stream)


def ptr(t):
    return None if t is None else _c_void_p(t.data_ptr())


def launch_count(family=None):
    if not available():
        return 0
    return int(_lib.p3d_launch_count() if family is None else _lib.p3d_launch_count_of(FAMILY[family]))


def i32x4(*v): return _i32x4(*v)
def i64x4(*v): return _i64x4(*v)
def i32x2(*v): return _i32x2(*v)
def i64x2(*v): return _i64x2(*v)


class kernel_timer:
    """``with kernel_timer('render_forward', tensor):`` brackets the enclosed launches with events on the tensor's
    current stream, but only while ``kernel_events['render_forward']`` exists — otherwise it costs one dict lookup."""

    def __init__(self, name, t):
        self.log = kernel_events.get(name)
        self.dev = t.device

    def __enter__(self):
        if self.log is not None:
            self.e0 = torch.cuda.Event(enable_timing=True)
            self.e0.record(torch.cuda.current_stream(self.dev))
        return self

    def __exit__(self, *exc):
        if self.log is not None:
            e1 = torch.cuda.Event(enable_timing=True)
            e1.record(torch.cuda.current_stream(self.dev))
            self.log.append((self.e0, e1))
