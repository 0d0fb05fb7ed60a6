"""Microseconds per call of the cross-view consistency primitives (pix2pix3d_amd/reproject.py) on an analytic-sphere scene (tests/reproject_cases.sphere_scene:
a sphere of radius 0.5 seen from 2.7 away by four cameras a few degrees apart, exact hit distances as depth), two ways on the same box:

(a) the device kernels of libp3d_regions.so: ``splat`` (each view into the next camera, radius 0 and 1, into a kept buffer refilled by every call),
    ``resolve`` (three channels, with target points and counts), ``difference_histogram`` (three channels under the status mask) and one
    ``Consistency.add`` of one pair (points, splat, two resolves, confusion, histogram);
(b) the same rule as torch ops on DEVICE tensors: the torch formulations of reproject.py (identical bytes, checked here before timing) — an int64
    ``scatter_reduce('amin')`` per footprint offset for the splat, a gather for the resolve, ``bincount`` under a boolean index (a host synchronisation) for
    the histogram.  Where the device does not support one of them the script says so and times the formulation on CPU tensors instead.

Sizes: [4, 128, 128] and [4, 512, 512].  Host clock around ``--calls`` calls that end in a device synchronise, after a warm-up, median and best of ``--reps``
repetitions; the variants are interleaved.

    python tools/bench_reproject.py [--reps 5] [--calls 50] [--out profiles/reproject_bench.json]

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
    from reproject_cases import sphere_scene
    from pix2pix3d_amd import evaluate, reproject
    assert torch.cuda.is_available(), 'bench_reproject.py measures the device kernels: it needs the GPU'
    dev = torch.device('cuda')
    angles = [(0.0, 0.0), (0.05, -0.02), (0.1, -0.05), (0.15, 0.0)]
    tol = round(0.02 * 65536)
    notes = []

    def add_torch(s, pts, pair, total):                                          # Consistency.add of one pair in torch ops on device tensors
        (i, j), f = pair, 1
        zbuf = torch.full([f, *pts.shape[1:3]], reproject.EMPTY, dtype=torch.int64, device=pts.device)
        reproject._splat_torch(pts[i:i + 1].reshape(1, -1, 3), s['cameras'][j:j + 1], None, 0, zbuf)
        labels, status, _ = reproject._resolve_torch(zbuf, s['labels'][i:i + 1, ..., None], [0], pts[j:j + 1], s['cameras'][j:j + 1], tol)
        images, _, _ = reproject._resolve_torch(zbuf, s['images'][i:i + 1], [0, 0, 0], None, None, None)
        total.status += torch.bincount(status.reshape(-1).long(), minlength=5)
        total.confusion += evaluate._confusion_torch(s['labels'][j:j + 1], labels[..., 0], 8, status == 1)
        total.differences += reproject._difference_histogram_torch(s['images'][j:j + 1], images, status[..., None], 1)

    rows = {}                                                                  # name -> (kernels, torch formulation, calls of the torch column, where it ran)
    for size in (128, 512):
        host = sphere_scene(angles, size)
        s = {k: v.to(dev) for k, v in host.items()}
        pts = reproject.points(s['depth'], s['cameras'])                         # the device's own points: the inputs of both columns
        pts_h = pts.cpu()
        cams_to, cams_to_h = s['cameras'].roll(-1, 0).contiguous(), host['cameras'].roll(-1, 0).contiguous()
        target, target_h = pts.roll(-1, 0).contiguous(), pts_h.roll(-1, 0).contiguous()
        tag = f'[4, {size}, {size}]'
        flat, flat_h = pts.reshape(4, -1, 3), pts_h.reshape(4, -1, 3)

        # identical bytes before any timing, and whether the device takes the torch formulation at all
        zbuf = reproject.splat(pts, cams_to)
        zbuf_h = reproject.splat(pts_h, cams_to_h)
        assert torch.equal(zbuf.cpu(), zbuf_h), tag
        assert torch.equal(reproject.splat(pts, cams_to, radius=1).cpu(), reproject.splat(pts_h, cams_to_h, radius=1)), tag
        where = 'torch_on_device'
        try:
            probe = reproject._splat_torch(flat, cams_to, None, 0, torch.full_like(zbuf, reproject.EMPTY))
            assert torch.equal(probe, zbuf), tag
        except (RuntimeError, NotImplementedError) as e:
            where = 'torch_on_cpu'
            notes.append(f'{tag}: int64 scatter_reduce(amin) on the device failed ({type(e).__name__}: {str(e).splitlines()[0][:120]}); the torch column of every row of this size is the CPU formulation')
        t = dict(pts=flat, cams=cams_to, target=target, images=s['images'], labels=s['labels'], zbuf=zbuf, scene=s, full=pts) if where == 'torch_on_device' else \
            dict(pts=flat_h, cams=cams_to_h, target=target_h, images=host['images'], labels=host['labels'], zbuf=zbuf_h, scene=host, full=pts_h)
        got = reproject.resolve(zbuf, s['images'], 0, target, cams_to, tol, return_index=True)
        want = reproject._resolve_torch(t['zbuf'], t['images'], [0, 0, 0], t['target'], t['cams'], tol)
        assert all(torch.equal(g.cpu(), w.cpu()) for g, w in zip(got, want)), tag
        warped, status = got[0], got[1]
        warped_t, status_t = want[0], want[1]
        images_to, images_to_t = s['images'].roll(-1, 0).contiguous(), t['images'].roll(-1, 0).contiguous()
        assert torch.equal(reproject.difference_histogram(images_to, warped, status, 1).cpu(),
                           reproject._difference_histogram_torch(images_to_t, warped_t, status_t[..., None], 1).cpu()), tag
        check, check_t = reproject.Consistency(8, dev), reproject.Consistency(8, t['pts'].device)
        check.add(s['labels'], s['images'], s['depth'], s['cameras'], [(0, 1)], tol)
        add_torch(t['scene'], t['full'], (0, 1), check_t)
        assert torch.equal(check._store.cpu(), check_t._store.cpu()), tag

        keep, keep_t = torch.empty_like(zbuf), torch.empty_like(t['zbuf'])
        counts, hist = torch.zeros(5, dtype=torch.int64, device=dev), torch.zeros(256, dtype=torch.int64, device=dev)
        total, total_t = reproject.Consistency(8, dev), reproject.Consistency(8, t['pts'].device)
        slow = max(1, args.calls // 10)
        for radius in (0, 1):
            rows[f'splat radius {radius} {tag}'] = (lambda r=radius, p=pts, c=cams_to, o=keep: reproject.splat(p, c, radius=r, out=o.fill_(reproject.EMPTY)),
                                                    lambda r=radius, p=t['pts'], c=t['cams'], o=keep_t: reproject._splat_torch(p, c, None, r, o.fill_(reproject.EMPTY)),
                                                    args.calls if where == 'torch_on_device' else slow, where)
        rows[f'resolve 3 channels, target points {tag}'] = (lambda z=zbuf, i=s['images'], p=target, c=cams_to, k=counts: reproject.resolve(z, i, 0, p, c, tol, counts=k),
                                                             lambda z=t['zbuf'], i=t['images'], p=t['target'], c=t['cams']: reproject._resolve_torch(z, i, [0, 0, 0], p, c, tol),
                                                             args.calls if where == 'torch_on_device' else slow, where)
        rows[f'difference_histogram 3 channels {tag}'] = (lambda a=images_to, b=warped, w=status, o=hist: reproject.difference_histogram(a, b, w, 1, out=o),
                                                           lambda a=images_to_t, b=warped_t, w=status_t[..., None]: reproject._difference_histogram_torch(a, b, w, 1),
                                                           args.calls if where == 'torch_on_device' else slow, where)
        rows[f'Consistency.add one pair [{size}, {size}]'] = (lambda q=s, o=total: o.add(q['labels'], q['images'], q['depth'], q['cameras'], [(0, 1)], tol),
                                                               lambda q=t['scene'], p=t['full'], o=total_t: add_torch(q, p, (0, 1), o), slow, where)

    def timed(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / calls

    us = {name: {'kernels': [], row[3]: []} for name, row in rows.items()}
    for kernel, composed, calls, where in rows.values():                       # warm-up: code objects, allocation sizes
        timed(kernel, 2)
        timed(composed, 2)
    for rep in range(args.reps):                                               # interleaved
        for name, (kernel, composed, calls, where) in rows.items():
            us[name]['kernels'].append(round(timed(kernel, calls), 1))
            us[name][where].append(round(timed(composed, calls), 1))

    print(f'{"us per call (median, best)":56s}{"kernels":>22s}{"torch formulation":>22s}')
    for name, cols in us.items():
        cell = lambda k: f'{np.median(cols[k]):9.1f} {min(cols[k]):9.1f}'
        other = [k for k in cols if k != 'kernels'][0]
        print(f'{name:56s}{cell("kernels"):>22s}{cell(other):>22s}  ({other})')
    for note in notes:
        print(note)
    line = {'workload': 'cross-view consistency on an analytic sphere (tests/reproject_cases.sphere_scene: radius 0.5, camera radius 2.7, focal 4.2647, four cameras; every view into the next)',
            'device': torch.cuda.get_device_name(0), 'calls_per_repetition': args.calls, 'us_per_call': us,
            'us_per_call_median': {n: {k: float(np.median(v)) for k, v in cols.items()} for n, cols in us.items()}, 'notes': notes,
            'not_measured': ['kernel times from a trace (the figures are host-clock times per call, launch overhead included)', 'radius 2 at 512 x 512',
                             'the contention case (every point on one pixel)'],
            'note': 'splat includes refilling the kept buffer (one fill launch) in both columns; resolve writes warped, status and counts; Consistency.add = points + splat + 2 resolves + confusion + histogram'}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
