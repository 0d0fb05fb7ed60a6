"""Time shape extraction on the GPU (pix2pix3d_amd/shape.py, csrc/shape.hip) and print ONE JSON line.

Config-size seg2cat and edge2car generators with seeded weights (configs.generator_kwargs, tests/golden/weights.py: no checkpoint is
needed).  Per config, device events after a warm-up:
  lattice_512_ms      one p3d_sample_lattice launch over 512^3 points (planes and decoder prepared once, outside the window)
  mc_512_ms           marching_cubes on that field (classify, scan, host copy of the totals, emit), at the script's threshold 50
                      and at the field's median
  extract_512_ms      extract_geometry(G, ws, 512, 50.0) end to end: backbone, lattice, marching cubes, rescale
  script_loop_ms      the script's get_sigma_field_np (extract_mesh.py:60-81): 512 x G.sample_mixed on 64^3 blocks on the device, each
                      block copied to the host
  lattice_256_ms / points_256_ms
                      the lattice launch against p3d_sample_points on the same 256^3 points as explicit coordinates, alternating
                      in one process (medians of the repetitions)
Usage: python tools/time_shape.py [--reps 5] [--configs seg2cat,edge2car]
"""
import argparse
import ctypes
import importlib.util
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from pix2pix3d_amd import _lib, configs, dnnlib, shape  # noqa: E402
from pix2pix3d_amd.training.volumetric_rendering import renderer as rmod  # noqa: E402


def _generator(name):
    spec = importlib.util.spec_from_file_location('p3d_weights', os.path.join(ROOT, 'tests', 'golden', 'weights.py'))
    weights = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(weights)
    torch.manual_seed(0)
    G = dnnlib.util.construct_class_by_name(**configs.generator_kwargs(name)).eval().requires_grad_(False)
    weights.seed_module(G, seed=1)
    return G.cuda()


def _ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def _median(fn, reps):
    fn()
    torch.cuda.synchronize()
    return statistics.median(_ms(fn)[0] for _ in range(reps))


def _script_loop(G, ws, resolution=512, block=64):
    bound = G.rendering_kwargs['box_warp'] * 0.5
    X = torch.linspace(-bound, bound, resolution).split(block)
    out = np.zeros([resolution] * 3, dtype=np.float32)
    for xi, xs in enumerate(X):
        for yi, ys in enumerate(X):
            for zi, zs in enumerate(X):
                xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing='ij')
                pts = torch.stack([xx, yy, zz], dim=-1).unsqueeze(0).to(ws.device)
                sig = G.sample_mixed(pts.reshape(1, -1, 3), None, ws=ws, noise_mode='const')['sigma']
                out[xi * block:xi * block + len(xs), yi * block:yi * block + len(ys), zi * block:zi * block + len(zs)] = \
                    sig.reshape(len(xs), len(ys), len(zs)).cpu().numpy()
    return out


def measure(name, reps):
    G = _generator(name)
    rk = G.rendering_kwargs
    ws = torch.randn([1, G.backbone.num_ws, 512], generator=torch.Generator().manual_seed(0)).cuda()
    lib = _lib.lib()
    with torch.no_grad():
        planes = shape._planes(G, ws, noise_mode='const')
        ctx = rmod._FusedContext(planes, rmod._decoder_nets(G.decoder))
        d = ctx.desc(rk)
        bound = rk['box_warp'] * 0.5

        def lattice(res):
            axis = torch.linspace(-bound, bound, res).cuda()
            sigma = torch.empty([1, res, res, res], device='cuda')

            def run():
                _lib.check(lib.p3d_sample_lattice(_lib.ptr(ctx.planes_cl), _lib.ptr(ctx.packed), ctypes.byref(d), *[_lib.ptr(axis)] * 3,
                                                  res, res, res, _lib.ptr(sigma), _lib.stream_of(sigma)), 'sample_lattice')
                return sigma
            return axis, sigma, run

        _, u512, run512 = lattice(512)
        r = {'lattice_512_ms': _median(run512, reps)}
        u = u512[0].clone()
        med = float(u.median())
        for key, thr in (('mc_512_ms', 50.0), ('mc_512_median_ms', med)):
            r[key] = _median(lambda: shape.marching_cubes(u, thr), reps)
            v, f = shape.marching_cubes(u, thr)
            r[key.replace('_ms', '_vertices')], r[key.replace('_ms', '_faces')] = int(v.shape[0]), int(f.shape[0])
        r['sigma_512_median'] = med
        r['extract_512_ms'] = _median(lambda: shape.extract_geometry(G, ws, 512, 50.0), reps)
        r['script_loop_ms'] = _ms(lambda: _script_loop(G, ws))[0]         # (the backbone and the point kernel are warm from the lines above)

        axis256, u256, run256 = lattice(256)
        xx, yy, zz = torch.meshgrid(axis256, axis256, axis256, indexing='ij')
        pts = torch.stack([xx, yy, zz], -1).reshape(1, -1, 3).contiguous()
        del xx, yy, zz
        p = pts.shape[1]
        rgb = torch.empty([1, p, 32 * ctx.n_nets], device='cuda')
        sig = torch.empty([1, p, 1], device='cuda')

        def points():
            _lib.check(lib.p3d_sample_points(_lib.ptr(ctx.planes_cl), _lib.ptr(ctx.packed), _lib.ptr(pts), ctypes.byref(d), p,
                                             _lib.ptr(rgb), _lib.ptr(sig), _lib.stream_of(sig)), 'sample_points')
            return sig
        run256()
        points()
        torch.cuda.synchronize()
        lat_t, pts_t = [], []
        for _ in range(reps):
            lat_t.append(_ms(run256)[0])
            pts_t.append(_ms(points)[0])
        r['lattice_256_ms'], r['points_256_ms'] = statistics.median(lat_t), statistics.median(pts_t)
        r['lattice_256_equals_points'] = bool(torch.equal(u256.reshape(-1), sig.reshape(-1)))
        r['n_nets'] = ctx.n_nets
    del G, planes, ctx, pts, rgb, sig
    torch.cuda.empty_cache()
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--configs', default='seg2cat,edge2car')
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'time_shape.py measures on the GPU'
    t0 = time.time()
    out = {'tool': 'time_shape', 'device': torch.cuda.get_device_name(0), 'reps': args.reps}
    for name in args.configs.split(','):
        out[name] = measure(name, args.reps)
    out['wall_s'] = round(time.time() - t0, 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
