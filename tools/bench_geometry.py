"""Geometry agreement on the seeded seg2cat mesh (threshold at the field's median, random weights as in bench.py), everything on the
device: the lattice's mesh against its ``mesh.simplify``-ed copy, per stage — ``surface_samples``, keys + sort, the tree build, ``closest``
with and without Morton-sorted queries on a given hierarchy, ``compare`` as a whole and ``mesh.simplify_to`` — and what a user had
before: the CPU definition and a torch-on-device brute force (``geometry.tri_d2`` on device tensors, all pairs in chunks) on a strided
subset whose pair count is stated, per pair.

    python tools/bench_geometry.py [--lattice 512] [--cell-steps 2] [--subset 256] [--reps 3] [--out profiles/geometry_bench.json]

Prints ONE JSON line: the sizes, the median wall time of every stage in ms over ``--reps`` repetitions after a warm-up (host timer
around a synchronised device), ns per pair of the two baselines and of the hierarchy's query.  No time is a pass condition."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lattice', type=int, default=512)
    ap.add_argument('--cell-steps', type=float, default=2.0, help="simplify's cell in lattice steps")
    ap.add_argument('--subset', type=int, default=256, help='query points of the baselines')
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from bench_texture import build
    from pix2pix3d_amd import _lib, geometry, mesh, shape
    dev = torch.device('cuda')
    G = build(dev)
    ws = torch.randn(1, G.backbone.num_ws, 512, generator=torch.Generator().manual_seed(1234)).to(dev)

    def timed(fn, reps=args.reps):
        out, times = None, []
        for k in range(reps + 1):                                      # the first call warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if k:
                times.append(1e3 * (time.perf_counter() - t0))
        return out, round(float(np.median(times)), 3)

    thr = float(shape.sigma_grid(G, ws, 64)[0].median())
    v, f = shape.extract_geometry(G, ws, args.lattice, thr)
    step = float(G.rendering_kwargs['box_warp']) / (args.lattice - 1)
    sv, sf = mesh.simplify(v, f, args.cell_steps * step)
    spacing = geometry.diagonal(v) / 512
    stage = {}
    samples, stage['surface_samples'] = timed(lambda: geometry.surface_samples(sv, sf, spacing))
    v32, f32 = geometry._mesh('bench', v, f)
    box = geometry._finite_box(v32)
    key = torch.empty([len(f32)], dtype=torch.int64, device=dev)

    def keys_and_sort():
        _lib.check(_lib.lib().p3d_mesh_bvh_keys(_lib.ptr(v32), len(v32), _lib.ptr(f32), len(f32), _lib.ptr(box), _lib.ptr(key),
                                                _lib.stream_of(v32)), 'mesh_bvh_keys')
        return torch.sort(key, stable=True).indices
    _, stage['keys_and_sort'] = timed(keys_and_sort)
    bvh, stage['build_bvh'] = timed(lambda: geometry.build_bvh(v, f))      # keys, sort and the level launches
    near, stage['closest_sorted_queries'] = timed(lambda: geometry.closest(samples.points, v, f, bvh=bvh, sort_queries=True))
    _, stage['closest_unsorted_queries'] = timed(lambda: geometry.closest(samples.points, v, f, bvh=bvh, sort_queries=False))
    agreement, stage['compare'] = timed(lambda: geometry.compare(v, f, sv, sf, spacing))
    tolerance = 2.0 * step
    picked, stage['simplify_to'] = timed(lambda: mesh.simplify_to(v, f, tolerance, spacing), reps=1)
    # the baselines: all pairs of a strided subset of the samples against every face
    sub = samples.points[::max(1, len(samples.points) // args.subset)][:args.subset]
    pairs = len(sub) * len(f)
    t0 = time.perf_counter()
    cpu = geometry.closest(sub.cpu(), v.cpu(), f.cpu())
    cpu_ms = 1e3 * (time.perf_counter() - t0)

    def brute():
        best = torch.full([len(sub)], float('inf'), dtype=torch.float64, device=dev)
        _, corners = geometry._corners(v32, f32)
        p = tuple(x[:, None] for x in sub.double().unbind(1))
        for f0 in range(0, len(f32), 1 << 14):
            a, b, c = (tuple(x[None, :] for x in corners[f0:f0 + (1 << 14), j].unbind(1)) for j in range(3))
            best = torch.minimum(best, geometry.tri_d2(p, a, b, c).min(1).values)
        return best
    dev_d2, brute_ms = timed(brute, reps=1)
    sub_near = geometry.closest(sub, v, f, bvh=bvh)
    assert torch.equal(sub_near.d2.cpu(), cpu.d2) and torch.equal(dev_d2.cpu(), cpu.d2)
    line = {'workload': f'seg2cat lattice-{args.lattice} mesh against simplify(cell = {args.cell_steps} steps)', 'device': torch.cuda.get_device_name(0),
            'vertices': len(v), 'faces': len(f), 'simplified_faces': len(sf), 'samples': len(samples.points), 'spacing': spacing, 'stage_ms': stage,
            'hausdorff': float(agreement.hausdorff), 'chamfer': float(agreement.chamfer), 'fscore': agreement.fscore.tolist(),
            'simplify_to': {'tolerance': tolerance, 'cell': picked[2], 'faces': len(picked[1])},
            'baseline': {'subset_points': len(sub), 'pairs': pairs, 'cpu_definition_ns_per_pair': round(1e6 * cpu_ms / pairs, 3),
                         'torch_device_brute_force_ns_per_pair': round(1e6 * brute_ms / pairs, 4),
                         'hierarchy_ns_per_pair_equivalent': round(1e6 * stage['closest_sorted_queries'] / (len(samples.points) * len(f)), 7)}}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
