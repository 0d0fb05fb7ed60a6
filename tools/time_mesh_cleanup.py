"""Time mesh clean-up on the GPU (pix2pix3d_amd/mesh.py, csrc/mesh_ops.hip), print ONE JSON line and write it to --out.

The seeded config-size seg2cat generator (configs.generator_kwargs, tests/golden/weights.py: no checkpoint is needed) and its mesh at
the median of the 512^3 density field (shape.extract_geometry), as tools/time_mesh_render.py.  Host clock around a call that ends in a
synchronise, medians of the repetitions after a warm-up:
  components_ms                       mesh.components (face range check, p3d_mesh_components, the int64 labels)
  clean_keep1_ms                      mesh.clean(keep=1): components, ranking and the stable compaction
  simplify_cell2_ms / _cell4_ms       mesh.simplify at cells of 2 and 4 lattice steps, on the whole mesh
  write_ply_*                         mesh.write_ply (host) of the mesh as extracted, after clean(keep=1), and after clean + simplify at 2 steps
  scipy_components_ms                 scipy.sparse.csgraph.connected_components on the same edges (host, if scipy imports), for scale
Usage: python tools/time_mesh_cleanup.py [--reps 5] [--out profiles/mesh_cleanup_time_mi355x.json]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pix2pix3d_amd import configs, dnnlib, mesh, shape  # noqa: E402


def _generator(name):
    spec = importlib.util.spec_from_file_location('p3d_weights', os.path.join(ROOT, 'tests', 'golden', 'weights.py'))
    weights = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(weights)
    torch.manual_seed(0)
    G = dnnlib.util.construct_class_by_name(**configs.generator_kwargs(name)).eval().requires_grad_(False)
    weights.seed_module(G, seed=1)
    return G.cuda()


def _median(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def _ply(path, v, f, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        mesh.write_ply(path, v, f)
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), os.path.getsize(path)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_cleanup_time_mi355x.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'time_mesh_cleanup.py measures on the GPU'
    t_start = time.time()
    out = {'tool': 'time_mesh_cleanup', 'device': torch.cuda.get_device_name(0), 'reps': args.reps}
    G = _generator('seg2cat')
    ws = torch.randn([1, G.backbone.num_ws, 512], generator=torch.Generator().manual_seed(0)).cuda()
    with torch.no_grad():
        thr = float(shape.sigma_grid(G, ws, 512)[0].median())
        v, f = shape.extract_geometry(G, ws, 512, thr)
    step = G.rendering_kwargs['box_warp'] / 511.0
    out.update(threshold=thr, lattice_step=step, vertices=int(v.shape[0]), faces=int(f.shape[0]))

    labels = mesh.components(f, len(v))
    out['components'] = int((labels == torch.arange(len(v), device=v.device)).sum())
    out['components_with_faces'] = int(labels[f[:, 0]].unique().numel())
    out['components_ms'] = _median(lambda: mesh.components(f, len(v)), args.reps)
    out['clean_keep1_ms'] = _median(lambda: mesh.clean(v, f, keep=1), args.reps)
    cv, cf, _ = mesh.clean(v, f, keep=1)
    out.update(clean_keep1_vertices=int(cv.shape[0]), clean_keep1_faces=int(cf.shape[0]))
    for steps in (2, 4):
        out[f'simplify_cell{steps}_ms'] = _median(lambda: mesh.simplify(v, f, steps * step), args.reps)
        sv, sf = mesh.simplify(v, f, steps * step)
        out.update({f'simplify_cell{steps}_vertices': int(sv.shape[0]), f'simplify_cell{steps}_faces': int(sf.shape[0])})
        del sv, sf
    sv, sf = mesh.simplify(cv, cf, 2 * step)
    out.update(clean_simplify_cell2_vertices=int(sv.shape[0]), clean_simplify_cell2_faces=int(sf.shape[0]))
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'mesh.ply')
        reps = max(1, args.reps // 2)
        out['write_ply_before_ms'], out['ply_before_bytes'] = _ply(path, v, f, reps)
        out['write_ply_clean_ms'], out['ply_clean_bytes'] = _ply(path, cv, cf, reps)
        out['write_ply_clean_simplify_cell2_ms'], out['ply_clean_simplify_cell2_bytes'] = _ply(path, sv, sf, reps)
    try:
        import numpy as np
        from scipy.sparse import coo_matrix
        from scipy.sparse.csgraph import connected_components
    except ImportError:
        out['scipy_components_ms'] = None
    else:
        fn = f.cpu().numpy()
        nv = len(v)

        def run():
            a = np.concatenate([fn[:, 0], fn[:, 1]])
            b = np.concatenate([fn[:, 1], fn[:, 2]])
            return connected_components(coo_matrix((np.ones(len(a), np.int8), (a, b)), shape=(nv, nv)), directed=False)[0]
        t0 = time.perf_counter()
        n_scipy = run()
        out['scipy_components_ms'] = (time.perf_counter() - t0) * 1e3      # seconds per call: one run
        out['scipy_components'] = int(n_scipy)
    out['wall_s'] = round(time.time() - t_start, 1)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
