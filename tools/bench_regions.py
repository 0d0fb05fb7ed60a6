"""Microseconds per call of the region tools (pix2pix3d_amd/regions.py) on the 512^2 random-blob mask of tests/edit_cases.random_mask (six labels), three ways on
the same box:

(a) the device kernels of libp3d_regions.so: ``components`` (4 / 8), ``nearest`` (radius 8 / unbounded), ``warp``, and the session operations
    (``EditSession.fill`` / ``grow`` / ``shrink`` / ``remove`` / ``scale``: append the entry, read ``s.mask``, ``undo()``);
(b) the same rule as torch ops on device tensors, where one exists: the torch formulations of regions.py (identical bytes, checked here before timing; the
    component and nearest ones read a flag back per iteration).  ``grow`` through ``max_pool2d`` is also timed but is NOT the same rule: its window is the
    (2 r + 1)^2 square, not the disc d^2 <= r^2, so its bytes differ and it is printed for scale only;
(c) the CPU formulation on host tensors.

Host clock around ``--calls`` calls that end in a device synchronise, after a warm-up, best and median of ``--reps`` repetitions; the variants are interleaved.

    python tools/bench_regions.py [--reps 5] [--calls 50] [--out profiles/regions_bench.json]

Prints a table and ONE JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from edit_cases import random_mask
    from pix2pix3d_amd import regions, configs
    assert torch.cuda.is_available(), 'bench_regions.py measures the device kernels: it needs the GPU'
    dev = torch.device('cuda')
    host = random_mask(1, 512, 512, 6, seed=0)[0]
    mask = host.to(dev)
    region_h = host == 2
    under_h = torch.where(region_h, 0, host).to(torch.uint8)
    region, under = region_h.to(dev).view(torch.uint8), under_h.to(dev)
    coef = regions.affine_coef([[1.3, 0, -70], [0, 1.3, -80]])
    words = regions.site_words({2})

    def square_grow(m, label, r):                                              # NOT the disc: for scale only
        on = (m == label).float()[None, None]
        return torch.where(torch.nn.functional.max_pool2d(on, 2 * r + 1, stride=1, padding=r)[0, 0] > 0, torch.tensor(label, dtype=torch.uint8, device=m.device), m)

    rows = {                                                                   # name -> (kernels, torch ops on the device or None, the CPU formulation)
        'components(4)': (lambda: regions.components(mask, 4), lambda: regions._components_torch(mask, 4), lambda: regions.components(host, 4)),
        'components(8)': (lambda: regions.components(mask, 8), lambda: regions._components_torch(mask, 8), lambda: regions.components(host, 8)),
        'nearest(radius 8)': (lambda: regions.nearest(mask, {2}, 8), lambda: regions._nearest_torch(mask, words, 8), lambda: regions.nearest(host, {2}, 8)),
        'nearest(unbounded)': (lambda: regions.nearest(mask, {2}, -1), lambda: regions._nearest_torch(mask, words, -1), lambda: regions.nearest(host, {2}, -1)),
        'warp': (lambda: regions.warp(mask, region, under, coef), lambda: regions._warp_torch(mask, region, under, coef),
                 lambda: regions.warp(host, region_h, under_h, coef)),
        'grow(8)': (lambda: regions.grow(mask, 2, 8), None, lambda: regions.grow(host, 2, 8)),
        'grow(8) max_pool2d square [not the same rule]': (None, lambda: square_grow(mask, 2, 8), None),
    }
    for name, (kernel, composed, cpu) in rows.items():                         # identical bytes before any timing
        if kernel is not None and cpu is not None:
            assert torch.equal(kernel().cpu(), cpu()), name
        if kernel is not None and composed is not None:
            assert torch.equal(kernel().to(torch.int64), composed().to(torch.int64)), name

    # ---- the session operations: append, read the mask, undo ---------------------------------------------------------------------------
    from bench_views import build
    from pix2pix3d_amd import edit
    G = build(dev)
    rk = G.rendering_kwargs
    pose = torch.from_numpy(configs.orbit_camera(9, radius=rk['avg_camera_radius'], pivot=rk['avg_camera_pivot']))
    s = edit.EditSession(G, cfg='seg2cat', seed=0, hold_texture=False)
    s.load(host, pose)
    by_hand = {'fill': lambda m: regions.flood_fill(m, 256, 256, 3), 'grow(8)': lambda m: regions.grow(m, 2, 8), 'shrink(4)': lambda m: regions.shrink(m, 2, 4),
               'remove': lambda m: regions.remove(m, 2), 'scale(1.3)': lambda m: regions.transform(m, m == 2, [[1.3, 0, 255.5 - 1.3 * 255.5], [0, 1.3, 255.5 - 1.3 * 255.5]])}
    ops = {'fill': lambda: s.fill(256, 256, 3), 'grow(8)': lambda: s.grow(2, 8), 'shrink(4)': lambda: s.shrink(2, 4), 'remove': lambda: s.remove(2),
           'scale(1.3)': lambda: s.scale(2, 1.3, centre=(255.5, 255.5))}

    def session_op(name):
        ops[name]()
        out = s.mask
        s.undo()
        return out
    for name in ops:
        assert torch.equal(session_op(name).cpu(), by_hand[name](host)), name
        rows[f'session {name}'] = ((lambda n=name: session_op(n)), None, (lambda n=name: by_hand[n](host)))

    def timed(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / calls

    us = {name: {} for name in rows}
    for name, fns in rows.items():
        for key, fn, calls in zip(('kernels', 'torch_on_device', 'cpu'), fns, (args.calls, max(1, args.calls // 10), max(1, args.calls // 10))):
            if fn is not None:
                timed(fn, 2)                                                    # warm-up: code objects, allocation sizes
                us[name][key] = []
    for rep in range(args.reps):                                               # interleaved
        for name, fns in rows.items():
            for key, fn, calls in zip(('kernels', 'torch_on_device', 'cpu'), fns, (args.calls, max(1, args.calls // 10), max(1, args.calls // 10))):
                if fn is not None:
                    us[name][key].append(round(timed(fn, calls), 1))

    print(f'{"us per call (median, best)":52s}{"kernels":>20s}{"torch ops, device":>22s}{"CPU formulation":>22s}')
    for name, cols in us.items():
        cell = lambda k: f'{np.median(cols[k]):9.1f} {min(cols[k]):9.1f}' if k in cols else '-'
        print(f'{name:52s}{cell("kernels"):>20s}{cell("torch_on_device"):>22s}{cell("cpu"):>22s}')
    line = {'workload': 'region tools on the 512^2 six-label random-blob mask (tests/edit_cases.random_mask, seed 0); label 2 as the region / the sites',
            'device': torch.cuda.get_device_name(0), 'calls_per_repetition': args.calls, 'us_per_call': us,
            'us_per_call_median': {n: {k: float(np.median(v)) for k, v in cols.items()} for n, cols in us.items()},
            'note': 'grow via max_pool2d dilates by the square, not the disc: different bytes, printed for scale only; session rows = append + s.mask + undo()'}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
