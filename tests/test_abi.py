"""The C-ABI shared library: loads without a GPU and exports every symbol include/*.h declares."""
import ctypes
import glob
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from conftest import ROOT


def _declared_symbols():
    names = set()
    for h in glob.glob(os.path.join(ROOT, 'include', '*.h')):
        src = re.sub(r'/\*.*?\*/', '', open(h).read(), flags=re.S)
        names |= set(re.findall(r'\b(p3d_[a-z0-9_]+)\s*\(', src))
    return sorted(names)


def test_library_loads_and_exports_every_declared_symbol():
    from pix2pix3d_amd import _lib
    handle = _lib.lib()                      # raises if the .so is missing or unresolved
    declared = _declared_symbols()
    assert len(declared) >= 6
    for name in declared:
        assert hasattr(handle, name), f'{name} declared in include/ but not exported'
    assert handle.p3d_abi_version() >= 1
    assert isinstance(_lib.launch_count(), int)


_KIND = {ctypes.c_void_p: 'ptr', ctypes.c_char_p: 'cstr', ctypes.c_int32: 'i32', ctypes.c_int64: 'i64', ctypes.c_uint32: 'u32', ctypes.c_uint64: 'u64',
         ctypes.c_float: 'f32', ctypes.c_double: 'f64'}
_PROBES_HEADER = os.path.join(ROOT, 'pix2pix3d_amd', 'csrc', 'probes', 'p3d_probes.h')
_STRUCT_SIZES = {'p3d_frame_job': 328, 'p3d_demod_job': 32, 'p3d_fc_job': 72, 'p3d_render_desc': 88}      # of the hand-written mirrors this binding replaced


def _probes_header():
    from pix2pix3d_amd import _lib
    return _lib.read_header(_PROBES_HEADER, base=_lib.HEADER)


# The prototypes the product header gained since the golden table was taken (a feature adds its row here), as the table writes them.
_SIGNATURES_SINCE = {'p3d_mesh_sample_counts': ['i32', 'ptr', 'i32', 'ptr', 'i32', 'f64', 'i32', 'ptr', 'ptr', 'ptr'],
                     'p3d_mesh_sample_points': ['i32', 'ptr', 'i32', 'ptr', 'i32', 'ptr', 'ptr', 'i64', 'ptr', 'ptr', 'ptr'],
                     'p3d_mesh_bvh_keys': ['i32', 'ptr', 'i32', 'ptr', 'i32', 'ptr', 'ptr', 'ptr'],
                     'p3d_mesh_bvh_build': ['i32', 'ptr', 'i32', 'ptr', 'i32', 'ptr', 'i32', 'ptr', 'ptr', 'ptr'],
                     'p3d_mesh_closest': ['i32', 'ptr', 'i64', 'ptr', 'ptr', 'i32', 'i32', 'ptr', 'ptr', 'ptr', 'ptr']}


def test_derived_signatures_equal_the_hand_written_table_they_replaced():
    """tests/golden/abi_signatures_parent.json: the 95 hand-written signatures of the last commit that had them plus the probe library's two, as
    name -> [restype kind, argument kinds...] (every pointer type a 'ptr', c_int an 'i32').  The header-derived table equalled it with no difference,
    so no entry is corrected.  What the header declares beyond it is pinned by ``_SIGNATURES_SINCE``: 102 signatures in all."""
    from pix2pix3d_amd import _lib
    with open(os.path.join(ROOT, 'tests', 'golden', 'abi_signatures_parent.json')) as f:
        want = json.load(f)
    assert len(want) == 97 and not set(want) & set(_SIGNATURES_SINCE)
    want.update(_SIGNATURES_SINCE)
    functions = {**_lib.HEADER.functions, **_probes_header().functions}
    got = {name: [_KIND[restype]] + [_KIND[a] for a in argtypes] for name, (restype, argtypes) in functions.items()}
    assert len(want) == 102 and sorted(got) == sorted(want)
    assert not {name: (got[name], want[name]) for name in want if got[name] != want[name]}


def test_every_declared_prototype_is_parsed_and_bound_by_importing_lib_alone():
    from pix2pix3d_amd import _lib
    declared = _declared_symbols()
    assert sorted(_lib.HEADER.functions) == declared and len(declared) >= 100
    child = ('import json, sys; from pix2pix3d_amd import _lib; raw = _lib.lib()._handle; '
             'print(json.dumps([n for n in sys.argv[1:] if getattr(raw, n).argtypes is None]))')
    r = subprocess.run([sys.executable, '-c', child] + declared, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1]) == []


def test_every_entry_point_the_package_calls_is_declared():
    """The source scan of the test this replaces (test_render_routes.py, "every module registers the entry points it calls"): with the signatures
    set from the header when the library is loaded (the test above), a call needs its name declared and nothing else — not an import of some module."""
    import pathlib
    from pix2pix3d_amd import _lib
    root = pathlib.Path(ROOT) / 'pix2pix3d_amd'
    probes = _probes_header().functions
    assert probes and not set(probes) & set(_lib.HEADER.functions)
    checked = []
    for path in sorted(root.rglob('*.py')):
        called = set(re.findall(r'\blib(?:\(\))?\.(p3d_\w+)', path.read_text()))
        declared = set(_lib.HEADER.functions) | (set(probes) if path.name == 'diagnostics.py' else set())
        checked += [path.name] * bool(called)
        assert called <= declared, (str(path.relative_to(root)), sorted(called - declared))
    assert len(checked) >= 9 and 'geometry.py' in checked


_LAYOUT_C = '''#include "%s"
#include <stddef.h>
#include <stdio.h>
int main(void) {
%s    return 0;
}
'''


_PRODUCT_HEADER = os.path.join(ROOT, 'include', 'p3d_hip.h')


def _compile_and_run(tmp_path, gcc, header, body):
    """The lines that a C program prints: ``body`` as the statements of a main() that includes ``header``."""
    src, exe = tmp_path / 'abi_probe.c', tmp_path / 'abi_probe'
    src.write_text(_LAYOUT_C % (header, body))
    r = subprocess.run([gcc, '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return [line.split() for line in r.stdout.splitlines()]


def test_struct_layouts_equal_the_c_compilers(tmp_path):
    from pix2pix3d_amd import _lib
    structs = _lib.HEADER.structs
    assert {name: ctypes.sizeof(c) for name, c in structs.items()} == _STRUCT_SIZES
    assert all(getattr(_lib, name) is c for name, c in structs.items())
    assert isinstance(_lib.p3d_frame_job().src_stride, ctypes.c_int64 * 4) and isinstance(_lib.p3d_frame_job().palette, ctypes.c_uint8 * 192)
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    body = ''
    for name, c in structs.items():
        body += f'    printf("{name} %zu\\n", sizeof({name}));\n'
        for field, _ in c._fields_:
            body += f'    printf("{name}.{field} %zu %zu\\n", offsetof({name}, {field}), sizeof((({name}*)0)->{field}));\n'
    got = {k: [int(x) for x in v] for k, *v in _compile_and_run(tmp_path, gcc, _PRODUCT_HEADER, body)}
    want = {name: [ctypes.sizeof(c)] for name, c in structs.items()}
    want.update({f'{name}.{field}': [getattr(c, field).offset, getattr(c, field).size] for name, c in structs.items() for field, _ in c._fields_})
    assert got == want and len(want) == 4 + 18 + 5 + 13 + 20


# the literals the package carried before it read them from the header, by the header's names
_CONSTANTS_BEFORE = {'P3D_OK': 0, 'P3D_ERR_UNSUPPORTED': -1, 'P3D_F32': 0, 'P3D_F16': 1, 'P3D_F64': 2, 'P3D_F32_BF16X3': 3, 'P3D_F32_BF16X6': 4,
                     'P3D_RENDER_SHARED_PLANES': 2, 'P3D_MESH_CAMERA_FLOATS': 24, 'P3D_MESH_GREY': 200, 'P3D_DEMOD_MAX_JOBS': 24, 'P3D_FC_MAX_JOBS': 40,
                     'P3D_FRAME_MAX_JOBS': 4, 'P3D_FRAME_SCALE': 0, 'P3D_FRAME_LABEL': 1, 'P3D_PAINT_MAX_SIZE': 4096, 'P3D_PAINT_MAX_STROKES': 65535,
                     'P3D_PAINT_MIN_COORD': -4096, 'P3D_PAINT_MAX_COORD': 8191}


def test_constants_equal_the_c_compilers_and_the_public_names_follow_them(tmp_path):
    import torch
    from pix2pix3d_amd import _lib, edit, mesh, views
    from pix2pix3d_amd.torch_utils.ops import modconv
    constants = _lib.HEADER.constants
    src = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'p3d_hip.h')).read(), flags=re.S)
    defines = set(re.findall(r'#\s*define\s+(P3D_\w+)[ \t]+\S', src))
    enumerators = {n for body in re.findall(r'\benum\b[^{;]*\{([^}]*)\}', src) for n in re.findall(r'\b(P3D_\w+)\b', body)}
    assert len(defines) >= 14 and len(enumerators) >= 35 and set(constants) == defines | enumerators
    assert all(getattr(_lib, name) == value for name, value in constants.items())
    assert {name: constants[name] for name in _CONSTANTS_BEFORE} == _CONSTANTS_BEFORE
    assert _lib.DTYPE_CODE == {torch.float32: 0, torch.float16: 1, torch.float64: 2}
    assert (mesh.CAMERA_FLOATS, mesh.GREY, views.MAX_JOBS, views.SCALE, views.LABEL) == (24, 200, 4, 0, 1)
    assert (edit.MAX_SIZE, edit.MAX_STROKES, edit.MIN_COORD, edit.MAX_COORD) == (4096, 65535, -4096, 8191)
    assert (modconv.FC_MAX_JOBS, modconv.DEMOD_MAX_JOBS, modconv.DTYPE_F32_BF16X3, modconv.DTYPE_F32_BF16X6) == (40, 24, 3, 4)
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    from pix2pix3d_amd import build
    side = {name: _lib.read_header(build.side_paths(name).header, base=_lib.HEADER) for name in build.SIDE_LIBRARIES}
    assert side['regions'].constants['P3D_VIEW_EMPTY'] == 2 ** 63 - 1 and len(side['regions'].constants) >= 15      # a suffixed literal among them
    for header, parsed in [(_PRODUCT_HEADER, constants)] + [(build.side_paths(name).header, side[name].constants) for name in side]:
        body = ''.join(f'    printf("{name} %lld\\n", (long long)({name}));\n' for name in sorted(parsed))
        assert {k: int(v) for k, v in _compile_and_run(tmp_path, gcc, header, body)} == parsed, header


def test_a_prototype_the_parser_cannot_type_is_an_error_that_names_it():
    from pix2pix3d_amd import _lib
    ok = _lib.Header('typedef void* p3d_stream_t;\nint p3d_fine(const float* x, int32_t n[2], double f, p3d_stream_t stream);')
    assert ok.functions == {'p3d_fine': (ctypes.c_int32, [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_double, ctypes.c_void_p])}
    for text, symbol, what in (('int p3d_fine(void);\nint p3d_odd(const float* x, unsigned n);', 'p3d_odd', 'unsigned'),
                               ('size_t p3d_sized(int n);', 'p3d_sized', 'size_t'),
                               ('int p3d_streamed(p3d_stream_t stream);', 'p3d_streamed', 'p3d_stream_t'),
                               ('typedef struct p3d_s { int32_t a; long b; } p3d_s;', 'p3d_s', 'long')):
        with pytest.raises(ValueError) as e:
            _lib.Header(text)
        assert symbol in str(e.value) and what in str(e.value), str(e.value)
    with pytest.raises(ValueError):
        _lib.Header('int p3d_fine(void);\nstatic inline int p3d_inline(int a) { return a; }')


def test_integer_constants_may_carry_a_c_suffix_and_nothing_else():
    from pix2pix3d_amd import _lib
    ok = _lib.Header('#define P3D_A 0x7fffffffffffffffLL\n#define P3D_B (-12l)\n#define P3D_C 7u\nenum { P3D_D = 5ULL, P3D_E, P3D_F = 0X1Flu };')
    assert ok.constants == {'P3D_A': 2 ** 63 - 1, 'P3D_B': -12, 'P3D_C': 7, 'P3D_D': 5, 'P3D_E': 6, 'P3D_F': 31}
    for text in ('#define P3D_A 0x7fLLx', '#define P3D_A 3lll', '#define P3D_A 1uu', 'enum { P3D_A = 0x7fLLx };'):
        with pytest.raises(ValueError):
            _lib.Header(text)


def test_argument_errors_are_reported_not_thrown():
    from pix2pix3d_amd import _lib
    h = _lib.lib()
    # null x: must come back as an error code + message, with no GPU work attempted
    code = h.p3d_bias_act(None, None, None, None, None, None, 0, 0, 1, 0.0, 1.0, -1.0, 16, 0, 1, None)
    assert code == -2
    assert b'non-null' in h.p3d_last_error()


def test_header_is_plain_c_and_a_c_client_links(tmp_path):
    """include/p3d_hip.h is the boundary a maintainer binds from C / cgo / JNI: it must compile as C99 (and C++) on its own, and a C
    translation unit that only includes it must link against libp3d_hip.so and be able to call the entry points that need no GPU."""
    import shutil
    import subprocess
    gcc = shutil.which('gcc')
    if gcc is None:
        pytest.skip('no gcc')
    hdr = os.path.join(ROOT, 'include', 'p3d_hip.h')
    for lang, std in (('c', 'c99'), ('c++', 'c++11')):
        r = subprocess.run([gcc, f'-std={std}', '-Wall', '-Wextra', '-pedantic', '-Werror', '-fsyntax-only', '-x', lang, hdr], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr
    src = tmp_path / 'client.c'
    src.write_text('#include "p3d_hip.h"\n#include <stdio.h>\n'
                   'int main(void) { printf("%d %d\\n", p3d_abi_version(), p3d_render_decoder_floats()); return p3d_abi_version() > 0 ? 0 : 1; }\n')
    exe = tmp_path / 'client'
    libdir = os.path.join(ROOT, 'pix2pix3d_amd')
    r = subprocess.run([gcc, '-std=c99', '-I', os.path.join(ROOT, 'include'), str(src), '-o', str(exe), '-L', libdir, '-lp3d_hip',
                        f'-Wl,-rpath,{libdir}', '-Wl,-rpath,/opt/rocm/lib'], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([str(exe)], capture_output=True, text=True, env=dict(os.environ, LD_LIBRARY_PATH=libdir + ':/opt/rocm/lib:' + os.environ.get('LD_LIBRARY_PATH', '')))
    from pix2pix3d_amd import _lib
    assert r.returncode == 0 and int(r.stdout.split()[0]) == _lib.lib().p3d_abi_version() >= 3, (r.stdout, r.stderr)
