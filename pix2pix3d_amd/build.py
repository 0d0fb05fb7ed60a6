"""Build libp3d_hip.so (the C-ABI kernel library) and the side libraries of ``SIDE_LIBRARIES`` in-tree with hipcc for gfx950.

No torch headers, no pybind: every ``csrc/*.hip`` translation unit is compiled to an object under ``csrc/_obj`` (in parallel, cached by mtime) and
linked into ``pix2pix3d_amd/libp3d_hip.so`` so the binary travels with the source tree to the GPU box.  A side library ``<name>`` is
``csrc/<name>/*.hip`` compiled into ``csrc/_obj/<name>/`` and linked with a copy of the library services (``_obj/p3d_common.o``) into
``pix2pix3d_amd/libp3d_<name>.so``: a library of its own, so that the product ABI of libp3d_hip.so gains no symbol.  hipcc cross-compiles without a
GPU present.
"""
import collections
import concurrent.futures
import os
import shutil
import subprocess
import sys

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, 'csrc')
OBJ_DIR = os.path.join(CSRC, '_obj')
LIB_PATH = os.path.join(PKG_DIR, 'libp3d_hip.so')
ARCH = 'gfx950'
CXXFLAGS = ['-O3', '-std=c++17', '-fPIC', f'--offload-arch={ARCH}', '-Wall', '-Wno-unused-function',
            '-fno-gpu-rdc', '-DNDEBUG']
# The libraries beside libp3d_hip.so, name -> extra compile flags.  Everything else about one follows from its name (side_paths).
SIDE_LIBRARIES = {'probes': ('-DP3D_BUILD_PROBES',),      # hardware probes the tests and the kernel studies use (diagnostics.py)
                  'regions': (),                         # region tools of the edit session, agreement metrics, cross-view reprojection (regions.py, evaluate.py, reproject.py)
                  'video': (),                           # everything on uint8 clips, held by clips.py: the frame writers and readers (video/), frame quality (quality.py, multiscale.py), resampling (resample.py)
                  'sketch': (),                          # edge-map canvas of the sketch session (sketch.py)
                  'mesh': ()}                            # quadric-error mesh decimation (decimate.py)
SidePaths = collections.namedtuple('SidePaths', 'src_dir header lib obj_dir')


def side_paths(name):
    """Where the side library ``name`` lives: the only statement of the convention (_lib.SideLibrary binds from the same paths)."""
    src_dir = os.path.join(CSRC, name)
    return SidePaths(src_dir, os.path.join(src_dir, f'p3d_{name}.h'), os.path.join(PKG_DIR, f'libp3d_{name}.so'), os.path.join(OBJ_DIR, name))


def _hipcc():
    for cand in (os.environ.get('HIPCC'), shutil.which('hipcc'), '/opt/rocm/bin/hipcc'):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError('hipcc not found: the gfx950 kernel library cannot be built')


def _newer(target, deps):
    if not os.path.exists(target):
        return False
    t = os.path.getmtime(target)
    return all(os.path.getmtime(d) <= t for d in deps)


def _files(directory, suffix):
    return sorted(os.path.join(directory, f) for f in os.listdir(directory) if f.endswith(suffix))


def sources():
    return _files(CSRC, '.hip')


def headers():
    dirs = [CSRC] + [side_paths(name).src_dir for name in SIDE_LIBRARIES] + [os.path.join(os.path.dirname(PKG_DIR), 'include')]
    return sorted(h for d in dirs for h in _files(d, '.h'))


def _object(src, obj_dir=OBJ_DIR):
    return os.path.join(obj_dir, os.path.basename(src)[:-4] + '.o')


def product_objects():
    """The objects libp3d_hip.so is linked from, in link order: one per ``csrc/*.hip``, nothing of a side library."""
    return [_object(src) for src in sources()]


def _run(cmd, verbose, what):
    if verbose:
        print(' '.join(cmd), flush=True)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'{what}:\n{r.stdout}')
    return r.stdout


def _compile(src, verbose, extra=(), obj_dir=OBJ_DIR):
    obj = _object(src, obj_dir)
    if _newer(obj, [src] + headers()):
        return obj, False
    os.makedirs(obj_dir, exist_ok=True)
    out = _run([_hipcc()] + CXXFLAGS + list(extra) + ['-c', src, '-o', obj], verbose, f'hipcc failed for {src}')
    if verbose and out.strip():
        print(out)
    return obj, True


def _compile_all(srcs, verbose, extra=(), obj_dir=OBJ_DIR):
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(8, len(srcs)))) as ex:
        return list(ex.map(lambda s: _compile(s, verbose, extra, obj_dir), srcs))


def _link(path, results, verbose):
    """Link the (object, recompiled) pairs into ``path`` unless it is newer than all of them."""
    objs = [o for o, _ in results]
    if any(changed for _, changed in results) or not _newer(path, objs):
        _run([_hipcc(), '-shared', '-fPIC', f'--offload-arch={ARCH}', '-o', path] + objs, verbose, 'link failed')
    return path


def build_library(force=False, verbose=False):
    """Compile + link libp3d_hip.so and every side library; returns the path of libp3d_hip.so."""
    if force:
        shutil.rmtree(OBJ_DIR, ignore_errors=True)
    _link(LIB_PATH, _compile_all(sources(), verbose), verbose)
    for name in SIDE_LIBRARIES:
        build_side(name, verbose=verbose)
    return LIB_PATH


def build_side(name, verbose=False):
    """libp3d_<name>.so: the sources of ``csrc/<name>`` with the product's flags plus the row's, and their own copy of the library services
    (``_obj/p3d_common.o``, compiled here if it is missing or stale: a side library builds on a clean tree by itself)."""
    paths = side_paths(name)
    common = _compile(os.path.join(CSRC, 'p3d_common.hip'), verbose)
    results = _compile_all(_files(paths.src_dir, '.hip'), verbose, SIDE_LIBRARIES[name], paths.obj_dir)
    return _link(paths.lib, results + [common], verbose)


if __name__ == '__main__':
    print(build_library(force='--force' in sys.argv, verbose=True))
