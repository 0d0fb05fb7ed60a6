"""Baking the views of one latent onto its extracted mesh, per stage: a lattice-512 seg2cat mesh (threshold at the field's median, random weights as in
bench.py), 24 views at 512^2, everything on the device — frames (``views.render_views``), project + rasterize (``mesh.project`` / ``mesh.rasterize``),
normals (``texture.vertex_normals``: the stable sort that builds the corner lists, and the kernel alone), accumulate (``p3d_mesh_bake_accumulate``, all views
in one launch per group) and finish — and the CPU formulation on a mesh small enough to finish (lattice 64, 4 views at 128^2).

    python tools/bench_texture.py [--lattice 512] [--views 24] [--reps 3] [--cpu-lattice 64] [--out profiles/texture_bench.json]

Prints ONE JSON line: the sizes, the median wall time of every stage in ms over ``--reps`` repetitions after a warm-up (host timer around a synchronised
device), the bytes the accumulate launch streams (records, vertex arrays, sums) with the rate that makes and the size of the buffers it gathers from,
and the CPU times.  No time is a pass condition."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(device):
    import importlib.util
    from pix2pix3d_amd import configs, dnnlib
    spec = importlib.util.spec_from_file_location('p3d_weights', os.path.join(ROOT, 'tests', 'golden', 'weights.py'))
    w = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(w)
    torch.manual_seed(0)
    G = dnnlib.util.construct_class_by_name(**configs.generator_kwargs('seg2cat', depth=(64, 64))).eval().requires_grad_(False)
    w.seed_module(G, seed=1)
    return G.to(device)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lattice', type=int, default=512)
    ap.add_argument('--views', type=int, default=24)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--cpu-lattice', type=int, default=64)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from pix2pix3d_amd import mesh, shape, texture, views
    dev = torch.device('cuda')
    G = build(dev)
    ws = torch.randn(1, G.backbone.num_ws, 512, generator=torch.Generator().manual_seed(1234)).to(dev)

    def timed(fn, reps=args.reps, sync=True):
        out, times = None, []
        for k in range(reps + 1):                                      # the first call warms up
            if sync:
                torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            if sync:
                torch.cuda.synchronize()
            if k:
                times.append(1e3 * (time.perf_counter() - t0))
        return out, round(float(np.median(times)), 3)

    thr = float(shape.sigma_grid(G, ws, 64)[0].median())
    v, f = shape.extract_geometry(G, ws, args.lattice, thr)
    cams = texture.bake_cameras(G, 'seg2cat', args.views).to(dev)
    c2w, cam = cams[:, :16].reshape(-1, 4, 4), mesh.Pinhole(cams[:, 16:25])
    stage = {}
    frames, stage['frames'] = timed(lambda: views.render_views(G, ws, cams, jitter='frozen', noise_mode='const', neural_rendering_resolution=128)['image'])
    size = frames.shape[1]
    (proj, fid, dep), stage['project_rasterize'] = timed(lambda: (lambda p: (p,) + mesh.rasterize(p, f, size))(mesh.project(v, c2w, cam, size)))
    normals, stage['normals'] = timed(lambda: texture.vertex_normals(v, f))
    _, stage['normals_corner_lists'] = timed(lambda: texture._corner_lists(f, len(v)))
    stage['normals_kernel'] = round(stage['normals'] - stage['normals_corner_lists'], 3)
    acc, seen = texture.bake_buffers(len(v), dev)

    def accumulate():
        acc.zero_(); seen.zero_()
        texture.bake_accumulate(acc, seen, proj, fid, dep, frames, v, normals, c2w)
    _, stage['accumulate'] = timed(accumulate)
    fallback = texture.vertex_rgb(G, ws, v)
    _, stage['finish'] = timed(lambda: texture.bake_finish(acc, fallback))
    _, stage['vertex_rgb'] = timed(lambda: texture.vertex_rgb(G, ws, v))
    _, stage['bake_colors_whole'] = timed(lambda: texture.bake_colors(v, f, frames, c2w, cam, fallback=fallback))
    # what one accumulate launch streams: every record once, positions, normals and the sums in and out.  The gathered buffers (ids, depths, frames)
    # are small enough to stay in the caches, so they are listed by their size, not by the bytes the gathers ask for
    n = len(v)
    streamed = n * args.views * 16 + n * (12 + 12 + 2 * 36)
    gathered = args.views * size * size * (4 + 4 + 3)

    # the CPU formulation on a small mesh
    vc, fc = shape.extract_geometry(G, ws, args.cpu_lattice, thr)
    vc, fc = vc.cpu(), fc.cpu()
    small = mesh.render(vc, fc, c2w[:4].cpu(), cam._replace(intrinsics=cams[:4, 16:25].cpu()), 128, colors=torch.full([len(vc), 3], 90, dtype=torch.uint8))
    cpu = {}
    _, cpu['normals'] = timed(lambda: texture.vertex_normals(vc, fc), reps=1, sync=False)
    _, cpu['bake_colors'] = timed(lambda: texture.bake_colors(vc, fc, small, c2w[:4].cpu(), cam._replace(intrinsics=cams[:4, 16:25].cpu())), reps=1, sync=False)

    line = {'workload': f'seg2cat lattice {args.lattice}, {args.views} views at {size}^2, pinhole video cameras', 'device': torch.cuda.get_device_name(0),
            'vertices': n, 'faces': len(f), 'seen_share': round(float((seen > 0).float().mean()), 4), 'views_per_seen_vertex': round(float(seen[seen > 0].float().mean()), 2),
            'stage_ms': stage, 'accumulate_streamed_bytes': streamed, 'accumulate_gathered_buffer_bytes': gathered,
            'accumulate_streamed_gb_per_s': round(streamed / (stage['accumulate'] * 1e-3) / 1e9, 1),
            'cpu': {'vertices': len(vc), 'faces': len(fc), 'views': 4, 'frame': 128, 'ms': cpu}}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
