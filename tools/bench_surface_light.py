"""What lighting a geometry frame costs beside the primary cast: the occlusion launch (``surface.occlusion``: ambient occlusion with 64 sphere
directions x 16 steps, shadows with 1 and with 8 rays towards the light x 64 steps) and the lit shade, each beside ``surface.cast`` of the
same run.  seg2cat as in tools/bench_surface.py (random weights as in bench.py), the threshold at the field's median, one camera of
``views.video_cameras`` per launch; the planes are made once, outside every timed window, as an edit session holds them.

    python tools/bench_surface_light.py [--resolution 512] [--steps 128] [--refine 8] [--views 4] [--reps 5] [--out FILE]

Prints ONE JSON line.  Per stage: ``ms`` (device events round the call — the launch with its operand preparation — median over reps x views
after a warm-up), ``ratio_to_cast`` (to cast.ms of this run) and ``evaluations``: the density evaluations the definition implies for one
camera, an upper bound on what the kernel runs — for the cast rays x steps + hits x (refine + 6), for an occlusion stage used rays x steps
(a blocked ray stops at its first dense sample, a ray that leaves the box stops there).  No number is a pass condition."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=512)
    ap.add_argument('--steps', type=int, default=128)
    ap.add_argument('--refine', type=int, default=8)
    ap.add_argument('--views', type=int, default=4)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from bench_texture import build
    from pix2pix3d_amd import shape, surface, views
    assert torch.cuda.is_available(), 'bench_surface_light.py measures on the GPU'
    dev = torch.device('cuda')
    G = build(dev)
    ws = torch.randn(1, G.backbone.num_ws, 512, generator=torch.Generator().manual_seed(1234)).to(dev)
    res, box = args.resolution, float(G.rendering_kwargs['box_warp'])
    light = (-0.5, -0.6, -0.6)
    with torch.no_grad():
        thr = float(shape.sigma_grid(G, ws, 64)[0].median())
        planes = shape._planes(G, ws, noise_mode='const')
        cams = views.video_cameras(G, 'seg2cat', max(args.views, 1)).to(dev)
        towards = surface.world_light(light, cams[:, :16], 'camera')
        sphere = surface.sphere_directions(64)
        cone = {n: surface.light_directions(towards, n, 0.1).to(dev) for n in (1, 8)}
        stages = {'ao_64x16': lambda k, hit: surface.occlusion(G, ws, hit, sphere, box / 4, steps=16, threshold=thr, planes=planes),
                  'shadow_1x64': lambda k, hit: surface.occlusion(G, ws, hit, cone[1][k:k + 1], box * math.sqrt(3.0), steps=64, threshold=thr, planes=planes),
                  'shadow_8x64': lambda k, hit: surface.occlusion(G, ws, hit, cone[8][k:k + 1], box * math.sqrt(3.0), steps=64, threshold=thr, planes=planes)}
        steps_of = {'ao_64x16': 16, 'shadow_1x64': 64, 'shadow_8x64': 64}

        def cast(k):
            return surface.cast(G, ws, cams[k:k + 1], res, steps=args.steps, refine=args.refine, threshold=thr, planes=planes)

        def shade(k, hit, pairs):
            return surface.shade_lit(hit, cams[k:k + 1, :16], None, towards[k:k + 1], pairs['ao_64x16'], pairs['shadow_8x64'])

        hit = cast(0)                                                    # warm-up: every shape of the timed windows
        shade(0, hit, {name: fn(0, hit) for name, fn in stages.items()})
        times = {name: [] for name in ('cast', 'shade_lit', *stages)}
        evals = {name: [] for name in ('cast', *stages)}
        hits = []
        for _ in range(args.reps):
            for k in range(args.views):
                hit, ms = event_ms(lambda: cast(k))
                times['cast'].append(ms)
                pairs = {}
                for name, fn in stages.items():
                    pairs[name], ms = event_ms(lambda: fn(k, hit))
                    times[name].append(ms)
                    evals[name].append(int(pairs[name][1].sum()) * steps_of[name])
                times['shade_lit'].append(event_ms(lambda: shade(k, hit, pairs))[1])
                n_hit = int(hit.hit.sum())
                hits.append(n_hit / (res * res))
                evals['cast'].append(res * res * args.steps + n_hit * (args.refine + 6))
    med = lambda t: float(np.median(t))
    cast_ms = med(times['cast'])
    line = {'workload': f'seg2cat, {res}^2 rays, cast {args.steps} steps + refine {args.refine}; {args.views} cameras one per launch, {args.reps} reps',
            'device': torch.cuda.get_device_name(0), 'threshold': round(thr, 4), 'hit_share': round(med(hits), 4)}
    for name, t in times.items():
        line[name] = {'ms': round(med(t), 3), 'ms_min_max': [round(min(t), 3), round(max(t), 3)], 'ratio_to_cast': round(med(t) / cast_ms, 3)}
        if name in evals:
            line[name]['evaluations'] = int(med(evals[name]))
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
