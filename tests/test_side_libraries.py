"""The kernel libraries beside libp3d_hip.so (``build.SIDE_LIBRARIES``), one row each: what the Python modules call is declared in the library's own
header, that header declares exactly what the library's sources define (the product's likewise), the headers are disjoint, every library exports its own
entry points and the product library none of them, ``SideLibrary.lib()`` binds every signature, and the library's own launch counter is wired.  No GPU is
needed — the argument checks run before any device call — but the built libraries are."""
import ctypes
import importlib
import os
import pathlib
import re

import pytest

from pix2pix3d_amd import build

ROOT = pathlib.Path(__file__).resolve().parent.parent
SERVICES = {'p3d_last_error', 'p3d_launch_count'}      # every side library links its own copy; their signatures come from the product header
# library -> (every module of pix2pix3d_amd that calls it; the accessor their calls go through; the module that holds the SideLibrary, where that is not the
# first caller: ``clips`` holds the video library and calls nothing itself).  A feature that adds entry points to a library adds its module here and its
# prototypes to the library's one header: never a second header or a binding of its own.
BOUND_BY = {'probes': (('diagnostics',), 'probes'), 'regions': (('regions', 'evaluate', 'reproject'), 'regions_lib'),
            'video': (('video.gif', 'video.jpeg', 'video.jpeg_read', 'video.png', 'quality', 'resample', 'multiscale'), 'video_lib', 'clips'),
            'sketch': (('sketch',), 'sketch_lib'), 'mesh': (('decimate',), 'mesh_lib')}
NAMES = sorted(build.SIDE_LIBRARIES)


def _module(name, k=0):
    return importlib.import_module('pix2pix3d_amd.' + BOUND_BY[name][0][k])


def _holder(name):
    return importlib.import_module('pix2pix3d_amd.' + BOUND_BY[name][2]) if len(BOUND_BY[name]) > 2 else _module(name)


def _exported(path, names):
    handle = ctypes.CDLL(str(path))
    return {n for n in names if hasattr(handle, n)}


@pytest.mark.parametrize('name', NAMES)
def test_calls_are_declared(name):
    module, accessor = _holder(name), BOUND_BY[name][1]
    assert getattr(module, accessor) == module._side.lib and module.HEADER is module._side.header
    declared = set(module.HEADER.functions)
    called_by_all = set()
    for k in range(len(BOUND_BY[name][0])):
        caller = _module(name, k)
        called = set(re.findall(r'\b%s\(\)\.(p3d_\w+)' % accessor, pathlib.Path(caller.__file__).read_text()))
        assert called - SERVICES and called - SERVICES <= declared, (name, caller.__name__, sorted(called - SERVICES - declared))
        called_by_all |= called - SERVICES
    assert called_by_all == declared, sorted(declared - called_by_all)          # every entry point has a caller among the modules of the row
    if name == 'video':
        from pix2pix3d_amd import video
        assert video._side is module._side and video.HEADER is module.HEADER and video.video_lib == module.video_lib


def _defined(sources):
    """The ``extern "C"`` p3d_* functions that .hip files define: ``extern "C" <type> p3d_x(`` and the definitions inside an ``extern "C" { }`` block
    (taken to run to the last closing brace at the start of a line)."""
    names = set()
    for path in sources:
        text = re.sub(r'/\*.*?\*/|//[^\n]*', '', pathlib.Path(path).read_text(), flags=re.S)
        names |= set(re.findall(r'extern\s+"C"\s+[\w\s*]+?\b(p3d_\w+)\s*\(', text))
        for block in re.findall(r'extern\s+"C"\s*\{(.*)^\}', text, flags=re.S | re.M):
            names |= set(re.findall(r'^[\w \t*]+?\b(p3d_\w+)\s*\([^;{]*\)\s*\{', block, flags=re.M))
    return names


def _declared(header):
    """As tests/test_abi.py scans include/*.h."""
    return set(re.findall(r'\b(p3d_[a-z0-9_]+)\s*\(', re.sub(r'/\*.*?\*/', '', pathlib.Path(header).read_text(), flags=re.S)))


@pytest.mark.parametrize('name', ['product'] + NAMES)
def test_the_header_declares_exactly_what_the_sources_define(name):
    """One header per library and nothing beside it: a function defined but not declared is bound by nobody (or by a second-hand binding), one declared but
    not defined fails the load.  A scan of the sources: no GPU, no built library.  A side library also links the services of p3d_common.hip, which the
    product header declares."""
    from pix2pix3d_amd import _lib
    services = _defined([os.path.join(build.CSRC, 'p3d_common.hip')])
    assert SERVICES <= services <= set(_lib.HEADER.functions)
    if name == 'product':
        defined, header = _defined(build.sources()), ROOT / 'include' / 'p3d_hip.h'
        assert len(defined) >= 100 and services <= defined
    else:
        paths = build.side_paths(name)
        defined, header = _defined(pathlib.Path(paths.src_dir).glob('*.hip')), paths.header
        assert defined and not defined & services
    assert defined == _declared(header), (sorted(defined - _declared(header)), sorted(_declared(header) - defined))


def test_only_the_six_headers_have_prototypes():
    own = [ROOT / 'include' / 'p3d_hip.h'] + [pathlib.Path(build.side_paths(name).header) for name in NAMES]
    assert [h for h in map(pathlib.Path, build.headers()) if h not in own and _declared(h)] == [] and all(_declared(h) for h in own)


@pytest.mark.parametrize('name', NAMES)
def test_headers_are_disjoint(name):
    from pix2pix3d_amd import _lib
    declared = set(_holder(name).HEADER.functions)
    assert declared and not declared & set(_lib.HEADER.functions)
    for other in NAMES:
        if other != name:
            assert not declared & set(_holder(other).HEADER.functions), (name, other)


@pytest.mark.parametrize('name', NAMES)
def test_exports_are_right(name):
    from pix2pix3d_amd import _lib
    module = _holder(name)
    declared = set(module.HEADER.functions)
    assert module._side.path == build.side_paths(name).lib
    assert _exported(module._side.path, declared | SERVICES) == declared | SERVICES
    assert _exported(_lib.LIB_PATH, declared) == set()                           # the product library gained no symbol


@pytest.mark.parametrize('name', NAMES)
def test_binding_is_complete(name):
    side = _holder(name)._side
    side.lib()
    assert [n for n in sorted(set(side.header.functions) | SERVICES) if getattr(side._raw, n).argtypes is None] == []


@pytest.mark.parametrize('name', NAMES)
def test_the_launch_counter_is_wired(name):
    """The first declared entry point with null pointers (1 for every integer: one frame, one pixel): its null check comes before any device call."""
    from pix2pix3d_amd import _lib
    side = _holder(name)._side
    n0 = side.launch_count()
    assert type(n0) is int
    fn_name, (_, argtypes) = next(iter(side.header.functions.items()))
    assert ctypes.c_void_p in argtypes
    code = getattr(side.lib(), fn_name)(*[None if t is ctypes.c_void_p else t(1) for t in argtypes])
    assert code == _lib.P3D_ERR_ARGUMENT == -2 and side.lib().p3d_last_error(), (fn_name, code)
    with pytest.raises(RuntimeError) as e:
        side.check(code, 'probe')
    assert str(e.value) == f'probe: libp3d_{name} error -2: {side.lib().p3d_last_error().decode()}'
    assert side.launch_count() == n0


def test_the_table_is_complete():
    """A directory of kernels without a row would silently be left out of the build."""
    with_kernels = {d.name for d in pathlib.Path(build.CSRC).iterdir() if d.is_dir() and list(d.glob('*.hip'))}
    assert with_kernels == set(build.SIDE_LIBRARIES) == set(BOUND_BY)
    for name in NAMES:
        paths = build.side_paths(name)
        assert os.path.isfile(paths.header) and paths.header in build.headers() and os.path.dirname(paths.obj_dir) == build.OBJ_DIR


def test_the_products_objects_are_the_products_only():
    objects = build.product_objects()
    assert [os.path.basename(o)[:-2] for o in objects] == [os.path.basename(s)[:-4] for s in build.sources()]
    assert sorted(os.path.basename(s) for s in build.sources()) == sorted(p.name for p in pathlib.Path(build.CSRC).glob('*.hip'))
    assert {os.path.dirname(o) for o in objects} == {build.OBJ_DIR}
    assert build.OBJ_DIR not in {build.side_paths(name).obj_dir for name in NAMES}


def test_the_load_error_is_unchanged(tmp_path):
    from pix2pix3d_amd import _lib
    side = _lib.SideLibrary('regions')
    side.path = str(tmp_path / 'libp3d_absent.so')
    with pytest.raises(OSError) as absent:
        ctypes.CDLL(side.path)
    with pytest.raises(RuntimeError) as e:
        side.lib()
    assert str(e.value) == f'pix2pix3d_amd: {side.path} could not be loaded ({absent.value}); build it with `python -m pix2pix3d_amd.build`'
    assert side._raw is None and side._guarded is None
