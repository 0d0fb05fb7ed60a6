"""Build libp3d_hip.so (the C-ABI kernel library), libp3d_probes.so, libp3d_regions.so, libp3d_video.so and libp3d_sketch.so in-tree with hipcc for gfx950.

No torch headers, no pybind: every ``csrc/*.hip`` translation unit is compiled to an object
(in parallel, cached by mtime) and linked into ``pix2pix3d_amd/libp3d_hip.so`` so the binary
travels with the source tree to the GPU box.  hipcc cross-compiles without a GPU present.
"""
import concurrent.futures
import os
import shutil
import subprocess
import sys

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(PKG_DIR, 'csrc')
OBJ_DIR = os.path.join(CSRC, '_obj')
LIB_PATH = os.path.join(PKG_DIR, 'libp3d_hip.so')
PROBES_DIR = os.path.join(CSRC, 'probes')
PROBES_LIB_PATH = os.path.join(PKG_DIR, 'libp3d_probes.so')      # hardware probes: a library of its own, never part of the product ABI
REGIONS_DIR = os.path.join(CSRC, 'regions')
REGIONS_LIB_PATH = os.path.join(PKG_DIR, 'libp3d_regions.so')    # region tools of the edit session: a library of its own too (csrc/regions/p3d_regions.h)
VIDEO_DIR = os.path.join(CSRC, 'video')
VIDEO_LIB_PATH = os.path.join(PKG_DIR, 'libp3d_video.so')        # palette, dither and index frames of the GIF writer: likewise (csrc/video/p3d_video.h)
SKETCH_DIR = os.path.join(CSRC, 'sketch')
SKETCH_LIB_PATH = os.path.join(PKG_DIR, 'libp3d_sketch.so')      # edge-map canvas of the sketch session: likewise (csrc/sketch/p3d_sketch.h)
ARCH = 'gfx950'
CXXFLAGS = ['-O3', '-std=c++17', '-fPIC', f'--offload-arch={ARCH}', '-Wall', '-Wno-unused-function',
            '-fno-gpu-rdc', '-DNDEBUG']


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


def sources():
    return sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.hip'))


def probe_sources():
    return sorted(os.path.join(PROBES_DIR, f) for f in os.listdir(PROBES_DIR) if f.endswith('.hip'))


def region_sources():
    return sorted(os.path.join(REGIONS_DIR, f) for f in os.listdir(REGIONS_DIR) if f.endswith('.hip'))


def video_sources():
    return sorted(os.path.join(VIDEO_DIR, f) for f in os.listdir(VIDEO_DIR) if f.endswith('.hip'))


def sketch_sources():
    return sorted(os.path.join(SKETCH_DIR, f) for f in os.listdir(SKETCH_DIR) if f.endswith('.hip'))


def headers():
    inc = os.path.join(os.path.dirname(PKG_DIR), 'include')
    hs = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith('.h')]
    hs += [os.path.join(PROBES_DIR, f) for f in os.listdir(PROBES_DIR) if f.endswith('.h')]
    hs += [os.path.join(REGIONS_DIR, f) for f in os.listdir(REGIONS_DIR) if f.endswith('.h')]
    hs += [os.path.join(VIDEO_DIR, f) for f in os.listdir(VIDEO_DIR) if f.endswith('.h')]
    hs += [os.path.join(SKETCH_DIR, f) for f in os.listdir(SKETCH_DIR) if f.endswith('.h')]
    hs += [os.path.join(inc, f) for f in os.listdir(inc) if f.endswith('.h')]
    return sorted(hs)


def _compile(src, verbose, extra=()):
    obj = os.path.join(OBJ_DIR, os.path.basename(src)[:-4] + '.o')
    if _newer(obj, [src] + headers()):
        return obj, False
    cmd = [_hipcc()] + CXXFLAGS + list(extra) + ['-c', src, '-o', obj]
    if verbose:
        print(' '.join(cmd), flush=True)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        raise RuntimeError(f'hipcc failed for {src}:\n{r.stdout}')
    if verbose and r.stdout.strip():
        print(r.stdout)
    return obj, True


def build_library(force=False, verbose=False):
    """Compile + link; returns the path of the shared library."""
    os.makedirs(OBJ_DIR, exist_ok=True)
    if force:
        for f in os.listdir(OBJ_DIR):
            os.remove(os.path.join(OBJ_DIR, f))
    srcs = sources()
    with concurrent.futures.ThreadPoolExecutor(max_workers=min(8, len(srcs))) as ex:
        results = list(ex.map(lambda s: _compile(s, verbose), srcs))
    objs = [o for o, _ in results]
    if any(changed for _, changed in results) or not _newer(LIB_PATH, objs):
        cmd = [_hipcc(), '-shared', '-fPIC', f'--offload-arch={ARCH}', '-o', LIB_PATH] + objs
        if verbose:
            print(' '.join(cmd), flush=True)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'link failed:\n{r.stdout}')
    build_probes(verbose=verbose)
    build_regions(verbose=verbose)
    build_video(verbose=verbose)
    build_sketch(verbose=verbose)
    return LIB_PATH


def _build_side_library(path, srcs, verbose, extra=()):
    """A library beside libp3d_hip.so: its own sources plus a copy of the library services (_obj/p3d_common.o, built by build_library)."""
    os.makedirs(OBJ_DIR, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(max_workers=max(1, min(8, len(srcs)))) as ex:
        results = list(ex.map(lambda s: _compile(s, verbose, extra), srcs))
    objs = [o for o, _ in results] + [os.path.join(OBJ_DIR, 'p3d_common.o')]
    if any(changed for _, changed in results) or not _newer(path, objs):
        cmd = [_hipcc(), '-shared', '-fPIC', f'--offload-arch={ARCH}', '-o', path] + objs
        if verbose:
            print(' '.join(cmd), flush=True)
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        if r.returncode != 0:
            raise RuntimeError(f'link failed:\n{r.stdout}')
    return path


def build_probes(verbose=False):
    """libp3d_probes.so (csrc/probes/*.hip, -DP3D_BUILD_PROBES): the hardware probes the tests and the kernel studies use, with their own
    copy of the library services (p3d_common.hip) so that nothing of them is exported through libp3d_hip.so."""
    return _build_side_library(PROBES_LIB_PATH, probe_sources(), verbose, ('-DP3D_BUILD_PROBES',))


def build_regions(verbose=False):
    """libp3d_regions.so (csrc/regions/*.hip): the region tools of pix2pix3d_amd/regions.py, with the same flags and their own copy of the
    library services; the product ABI of libp3d_hip.so gains no symbol."""
    return _build_side_library(REGIONS_LIB_PATH, region_sources(), verbose)


def build_video(verbose=False):
    """libp3d_video.so (csrc/video/*.hip): the palette kernels of pix2pix3d_amd/video.py, built as the region tools are; the product ABI of
    libp3d_hip.so gains no symbol."""
    return _build_side_library(VIDEO_LIB_PATH, video_sources(), verbose)


def build_sketch(verbose=False):
    """libp3d_sketch.so (csrc/sketch/*.hip): the canvas kernels of pix2pix3d_amd/sketch.py, built as the region tools are; the product ABI of
    libp3d_hip.so gains no symbol."""
    return _build_side_library(SKETCH_LIB_PATH, sketch_sources(), verbose)


if __name__ == '__main__':
    print(build_library(force='--force' in sys.argv, verbose=True))
