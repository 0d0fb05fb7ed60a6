"""Microseconds per call of the sketch tools (pix2pix3d_amd/sketch.py) at 128^2 and 512^2, two ways on the same box:

(a) the device path: the kernels of libp3d_sketch.so on device tensors (``link`` and ``edges`` with the three launches of ``regions.components``);
(b) the host route a caller without them takes: the CPU formulation on host tensors and the copy of its result to the device.

Inputs: ``condition`` and ``thin`` / ``trace`` on a canvas of one-pixel lines (tests/sketch_cases.crossing_lines; ``trace`` on its blur), the edge functions on
the seeded picture of tests/sketch_cases.random_rgb.  Identical bytes are checked before any timing.  Host clock around ``--calls`` calls that end in a device
synchronise, after a warm-up, best and median of ``--reps`` repetitions; the variants are interleaved.

    python tools/bench_sketch.py [--reps 5] [--calls 50] [--out profiles/sketch_bench.json]

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
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--calls', type=int, default=50)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from sketch_cases import crossing_lines, random_rgb
    from pix2pix3d_amd import sketch
    assert torch.cuda.is_available(), 'bench_sketch.py measures the device kernels: it needs the GPU'
    dev = torch.device('cuda')

    rows = {}                                                                  # name -> (device path, host route)
    for size in (128, 512):
        ink_h, rgb_h = crossing_lines(size, size), random_rgb(size, size, seed=size)
        soft_h = sketch.blur3(ink_h)
        classes_h = sketch.edge_classes(rgb_h, 60, 240)
        ink, rgb, soft, classes = ink_h.to(dev), rgb_h.to(dev), soft_h.to(dev), classes_h.to(dev)
        table = sketch.condition_table('dataset')
        table_d = table.to(dev)
        cases = {
            'condition -> 128^2': (lambda a=ink, t=table_d: sketch.condition(a, 128, table=t), lambda a=ink_h, t=table: sketch.condition(a, 128, table=t)),
            'edge_classes (RGB, smooth)': (lambda a=rgb: sketch.edge_classes(a, 60, 240), lambda a=rgb_h: sketch.edge_classes(a, 60, 240)),
            'link': (lambda a=classes: sketch.link(a), lambda a=classes_h: sketch.link(a)),
            'edges': (lambda a=rgb: sketch.edges(a, 60, 240), lambda a=rgb_h: sketch.edges(a, 60, 240)),
            'trace (2 passes)': (lambda a=soft: sketch.trace(a), lambda a=soft_h: sketch.trace(a)),
        }
        for name, (device_path, cpu) in cases.items():
            assert torch.equal(device_path().cpu(), cpu()), (size, name)       # identical bytes before any timing
            rows[f'{size}^2 {name}'] = (device_path, lambda f=cpu: f().to(dev))

    def timed(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / calls

    keys, calls = ('kernels', 'host_route'), (args.calls, max(1, args.calls // 10))
    us = {name: {k: [] for k in keys} for name in rows}
    for fns in rows.values():
        for fn in fns:
            timed(fn, 2)                                                        # warm-up: code objects, allocation sizes
    for rep in range(args.reps):                                               # interleaved
        for name, fns in rows.items():
            for key, fn, n in zip(keys, fns, calls):
                us[name][key].append(round(timed(fn, n), 1))

    print(f'{"us per call (median, best)":44s}{"device path":>22s}{"CPU formulation + copy":>26s}')
    for name, cols in us.items():
        cell = lambda k: f'{np.median(cols[k]):9.1f} {min(cols[k]):9.1f}'
        print(f'{name:44s}{cell("kernels"):>22s}{cell("host_route"):>26s}')
    line = {'workload': 'sketch tools at 128^2 and 512^2: a canvas of one-pixel lines (condition, trace), a seeded random picture (edge_classes, link, edges); thresholds 60 / 240',
            'device': torch.cuda.get_device_name(0), 'calls_per_repetition': args.calls, 'us_per_call': us,
            'us_per_call_median': {n: {k: float(np.median(v)) for k, v in cols.items()} for n, cols in us.items()},
            'note': 'host clock; device path = the calls of sketch.py on device tensors (link / edges include the three launches of regions.components and the '
                    'allocations); host route = the CPU formulation on host tensors plus the copy of the result to the device'}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
