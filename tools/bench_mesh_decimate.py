"""Time quadric-error decimation on the GPU (pix2pix3d_amd/decimate.py, csrc/mesh/mesh_decimate.hip) against vertex clustering, print ONE JSON line
and write it to --out.

The mesh of tools/time_mesh_cleanup.py: the seeded config-size seg2cat generator at the median of its density field on a --resolution^3 lattice
(default 512), largest component.  For each of 1/4 and 1/16 of its faces:
  decimate_ms, rounds, faces           decimate.decimate to that target (host clock around a call that ends in a synchronise; the median of --reps)
  kernels_ms                           of one more, instrumented call: the time inside the four entry points (a synchronise before and after each), the rest
                                       being the sorts and scans of torch that rebuild the lists every round
  simplify_ms, simplify_faces, cell    mesh.simplify at the coarsest cell of the ladder 0.97^i diagonal / 2 that yields at least as many faces
  *_hausdorff, *_chamfer               geometry.compare of each result with the input (sampled symmetric Hausdorff and Chamfer distances, --spacing-div:
                                       spacing = diagonal / that)
Usage: python tools/bench_mesh_decimate.py [--reps 3] [--resolution 512] [--out profiles/mesh_decimate_mi355x.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pix2pix3d_amd import decimate, geometry, mesh, shape  # noqa: E402
from tools.time_mesh_cleanup import _generator  # noqa: E402


def _timed(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts), out


def _kernel_time(fn):
    """The time ``fn`` spends inside the entry points of decimate.py, by wrapping them for one call."""
    spent = [0.0]
    names = ('quadrics', 'edge_costs', 'edge_select', 'collapse')
    originals = {name: getattr(decimate, name) for name in names}

    def wrap(inner):
        def run(*args):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = inner(*args)
            torch.cuda.synchronize()
            spent[0] += (time.perf_counter() - t0) * 1e3
            return out
        return run
    try:
        for name in names:
            setattr(decimate, name, wrap(originals[name]))
        fn()
    finally:
        for name in names:
            setattr(decimate, name, originals[name])
    return spent[0]


def _distances(v, f, out_v, out_f, spacing):
    agreement = geometry.compare(v, f, out_v, out_f, spacing)
    return float(agreement.hausdorff), float(agreement.chamfer)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--resolution', type=int, default=512)
    ap.add_argument('--spacing-div', type=float, default=512.0)
    ap.add_argument('--fraction', type=float, default=0.25)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'mesh_decimate_mi355x.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_mesh_decimate.py measures on the GPU'
    t_start = time.time()
    out = {'tool': 'bench_mesh_decimate', 'device': torch.cuda.get_device_name(0), 'reps': args.reps, 'resolution': args.resolution,
           'fraction': args.fraction}
    G = _generator('seg2cat')
    ws = torch.randn([1, G.backbone.num_ws, 512], generator=torch.Generator().manual_seed(0)).cuda()
    with torch.no_grad():
        thr = float(shape.sigma_grid(G, ws, args.resolution)[0].median())
        v, f = shape.extract_geometry(G, ws, args.resolution, thr)
    v, f, _ = mesh.clean(v, f, keep=1)
    diagonal = geometry.diagonal(v)
    spacing = diagonal / args.spacing_div
    out.update(vertices=int(v.shape[0]), faces=int(f.shape[0]), diagonal=diagonal, spacing=spacing, cases=[])
    decimate.decimate(v, f, len(f) - 64)                                     # warm-up: loads the library, sizes the allocator's pools
    for divisor in (4, 16):
        target = len(f) // divisor
        case = {'target_faces': target}
        case['decimate_ms'], result = _timed(lambda: decimate.decimate(v, f, target, args.fraction), args.reps)
        case.update(rounds=result.rounds, reached=result.reached, faces=int(result.faces.shape[0]), vertices=int(result.vertices.shape[0]))
        case['kernels_ms'] = _kernel_time(lambda: decimate.decimate(v, f, target, args.fraction))
        case['decimate_hausdorff'], case['decimate_chamfer'] = _distances(v, f, result.vertices, result.faces, spacing)
        for i in range(400):                                                # the coarsest cell with at least as many faces
            cell = 0.97 ** i * diagonal / 2
            sv, sf = mesh.simplify(v, f, cell)
            if len(sf) >= len(result.faces):
                break
        case['simplify_ms'], _ = _timed(lambda: mesh.simplify(v, f, cell), args.reps)
        case.update(cell=cell, simplify_faces=int(sf.shape[0]), simplify_vertices=int(sv.shape[0]))
        case['simplify_hausdorff'], case['simplify_chamfer'] = _distances(v, f, sv, sf, spacing)
        out['cases'].append(case)
        print(json.dumps(case), file=sys.stderr, flush=True)
        del result, sv, sf
    out['wall_s'] = round(time.time() - t_start, 1)
    line = json.dumps(out)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write(line + '\n')


if __name__ == '__main__':
    main()
