"""The mesh filters on the seeded seg2cat mesh, per stage and per lattice (threshold at the field's median, random weights as in bench.py), everything
on the device: ``mesh.adjacency`` (sorts and uniques in torch), 10 Taubin iterations (``mesh.smooth``: 20 launches of p3d_mesh_smooth_step on a given
adjacency), 2 voting steps (``mesh.smooth_labels``), ``texture.vertex_normals`` of the smoothed mesh, and the script's 120-frame 512^2 turntable with
flat and with smooth shading (``mesh.render``).

    python tools/bench_mesh_filter.py [--lattices 128 512] [--frames 120] [--reps 3] [--out profiles/mesh_filter_bench.json]

Prints ONE JSON line: per lattice the sizes, the largest degree and the median wall time of every stage in ms over ``--reps`` repetitions after a
warm-up (host timer around a synchronised device), and what one smoothing step of ``smooth`` takes (the call's time over its 20 steps) against the
bytes of its arrays, each counted once (positions in and out, pinned, offsets, the lists; the gathered neighbour rows are re-reads of the positions).
No time is a pass condition."""
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
    ap.add_argument('--lattices', type=int, nargs='+', default=[128, 512])
    ap.add_argument('--frames', type=int, default=120)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from bench_texture import build
    from pix2pix3d_amd import mesh, shape, texture
    dev = torch.device('cuda')
    G = build(dev)
    ws = torch.randn(1, G.backbone.num_ws, 512, generator=torch.Generator().manual_seed(1234)).to(dev)

    def timed(fn):
        out, times = None, []
        for k in range(args.reps + 1):                                 # the first call warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if k:
                times.append(1e3 * (time.perf_counter() - t0))
        return out, round(float(np.median(times)), 3)

    thr = float(shape.sigma_grid(G, ws, 64)[0].median())
    poses, camera = mesh.script_turntable(G, args.frames)
    results = []
    for lattice in args.lattices:
        v, f = shape.extract_geometry(G, ws, lattice, thr)
        labels = mesh.vertex_labels(G, ws, v)[0]
        stage = {}
        adj, stage['adjacency'] = timed(lambda: mesh.adjacency(f, len(v)))
        smoothed, stage['smooth_10_iterations'] = timed(lambda: mesh.smooth(v, f, 10, adjacency=adj))
        _, stage['smooth_labels_2_steps'] = timed(lambda: mesh.smooth_labels(labels, f, 2, int(G.semantic_channels), adjacency=adj))
        normals, stage['vertex_normals'] = timed(lambda: texture.vertex_normals(smoothed, f))
        _, stage['turntable_flat'] = timed(lambda: mesh.render(smoothed, f, poses, camera, 512))
        _, stage['turntable_smooth'] = timed(lambda: mesh.render(smoothed, f, poses, camera, 512, normals=normals))
        n, e = len(v), int(adj.neighbours.shape[0])
        step_ms = stage['smooth_10_iterations'] / 20
        step_bytes = n * (12 + 12 + 1 + 8) + e * 4                      # each array once: rows in and out, pinned, offsets, the lists
        results.append({'lattice': lattice, 'vertices': n, 'faces': len(f), 'list_entries': e,
                        'max_degree': int(adj.offsets.diff().max()) if n else 0, 'boundary_vertices': int(adj.boundary.sum()), 'stage_ms': stage,
                        'smooth_step_ms': round(step_ms, 4), 'smooth_step_bytes': step_bytes, 'smooth_step_gb_per_s': round(step_bytes / (step_ms * 1e-3) / 1e9, 1)})
    line = {'workload': f'seg2cat mesh filters, {args.frames}-frame 512^2 turntable', 'device': torch.cuda.get_device_name(0), 'runs': results}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
