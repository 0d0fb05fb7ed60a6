"""Microseconds per call of the agreement metrics (pix2pix3d_amd/evaluate.py) on random-blob label maps (tests/edit_cases.random_mask; the prediction
agrees with the truth on about 70 % of the pixels), two ways on the same box:

(a) the device kernels of libp3d_regions.so: ``confusion`` (ONE ``p3d_label_confusion`` launch over all frames, into a kept counter), ``boundary`` and
    ``distance_histogram`` (one launch each, one frame) and ``Agreement.add`` (confusion + the class-agnostic boundary counts of every frame);
(b) the same rule as torch ops on device tensors: the torch formulations of evaluate.py (identical counts, checked here before timing) — ``bincount`` of
    int64 keys for the confusion matrix, shifted compares for the boundary, ``bincount`` under a boolean index (a host synchronisation) for the histogram;
    for ``Agreement.add`` those three with ``regions._nearest_torch``.

Sizes: [4, 512, 512] with 6 and with 19 labels, and [8, 128, 128] with 6.  Host clock around ``--calls`` calls that end in a device synchronise, after a
warm-up, best and median of ``--reps`` repetitions; the variants are interleaved.

    python tools/bench_evaluate.py [--reps 5] [--calls 50] [--out profiles/evaluate_bench.json]

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
    from edit_cases import random_mask
    from pix2pix3d_amd import evaluate, regions
    assert torch.cuda.is_available(), 'bench_evaluate.py measures the device kernels: it needs the GPU'
    dev = torch.device('cuda')
    every = evaluate.CLASS_AGNOSTIC
    words = regions.site_words(every)

    def add_torch(truth, pred, n_labels, counts, hist):                          # Agreement.add in torch ops on device tensors
        counts += evaluate._confusion_torch(truth, pred, n_labels, None)
        for t, p in zip(truth, pred):
            bt, bp = evaluate._boundary_torch(t), evaluate._boundary_torch(p)
            near_t, near_p = regions._nearest_torch(bt, words, -1), regions._nearest_torch(bp, words, -1)
            hist[0] += evaluate._distance_histogram_torch(bp, words, near_t, 65)
            hist[1] += evaluate._distance_histogram_torch(bt, words, near_p, 65)

    rows = {}                                                                  # name -> (kernels, torch ops on the device, calls of the torch column)
    for (n, h, w), n_labels in (((4, 512, 512), 6), ((4, 512, 512), 19), ((8, 128, 128), 6)):
        truth_h, other = random_mask(n, h, w, n_labels, seed=0), random_mask(n, h, w, n_labels, seed=1)
        pred_h = torch.where(torch.rand(n, h, w, generator=torch.Generator().manual_seed(2)) < 0.7, truth_h, other)
        truth, pred = truth_h.to(dev), pred_h.to(dev)
        tag = f'[{n}, {h}, {w}] {n_labels} labels'
        counts = torch.zeros(n_labels * n_labels + 1, dtype=torch.int64, device=dev)
        bt, bp = evaluate.boundary(truth[0]), evaluate.boundary(pred[0])
        near = regions.nearest(bt, every)
        hist = torch.zeros(67, dtype=torch.int64, device=dev)
        total = evaluate.Agreement(n_labels, dev)
        t_counts, t_hist = torch.zeros_like(counts), torch.zeros(2, 67, dtype=torch.int64, device=dev)

        # identical counts before any timing
        assert torch.equal(evaluate.confusion(truth, pred, n_labels), evaluate._confusion_torch(truth, pred, n_labels, None)), tag
        assert torch.equal(evaluate.confusion(truth, pred, n_labels).cpu(), evaluate.confusion(truth_h, pred_h, n_labels)), tag
        assert torch.equal(bt, evaluate._boundary_torch(truth[0])), tag
        assert torch.equal(evaluate.distance_histogram(bp, every, near, 65), evaluate._distance_histogram_torch(bp, words, near, 65)), tag
        check, check_t = evaluate.Agreement(n_labels, dev), (torch.zeros_like(counts), torch.zeros_like(t_hist))
        check.add(truth, pred)
        add_torch(truth, pred, n_labels, *check_t)
        assert torch.equal(check.counts, check_t[0]) and torch.equal(check.boundary, check_t[1]), tag

        rows[f'confusion {tag}'] = (lambda a=truth, b=pred, c=n_labels, o=counts: evaluate.confusion(a, b, c, out=o),
                                    lambda a=truth, b=pred, c=n_labels, o=t_counts: o.add_(evaluate._confusion_torch(a, b, c, None)), args.calls)
        rows[f'boundary [{h}, {w}] {n_labels} labels'] = (lambda m=truth[0]: evaluate.boundary(m), lambda m=truth[0]: evaluate._boundary_torch(m), args.calls)
        rows[f'distance_histogram [{h}, {w}] {n_labels} labels'] = (lambda m=bp, q=near, o=hist: evaluate.distance_histogram(m, every, q, 65, out=o),
                                                                    lambda m=bp, q=near: evaluate._distance_histogram_torch(m, words, q, 65), args.calls)
        rows[f'Agreement.add {tag}'] = (lambda a=truth, b=pred, t=total: t.add(a, b),
                                        lambda a=truth, b=pred, c=n_labels, o=t_counts, g=t_hist: add_torch(a, b, c, o, g), max(1, args.calls // 10))

    def timed(fn, calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e6 / calls

    us = {name: {'kernels': [], 'torch_on_device': []} for name in rows}
    for kernel, composed, calls in rows.values():                              # warm-up: code objects, allocation sizes
        timed(kernel, 2)
        timed(composed, 2)
    for rep in range(args.reps):                                               # interleaved
        for name, (kernel, composed, calls) in rows.items():
            us[name]['kernels'].append(round(timed(kernel, calls), 1))
            us[name]['torch_on_device'].append(round(timed(composed, calls), 1))

    print(f'{"us per call (median, best)":52s}{"kernels":>22s}{"torch ops, device":>22s}')
    for name, cols in us.items():
        cell = lambda k: f'{np.median(cols[k]):9.1f} {min(cols[k]):9.1f}'
        print(f'{name:52s}{cell("kernels"):>22s}{cell("torch_on_device"):>22s}')
    line = {'workload': 'agreement metrics on random-blob label maps (tests/edit_cases.random_mask, seeds 0 / 1; the prediction equals the truth on 70 % of the pixels)',
            'device': torch.cuda.get_device_name(0), 'calls_per_repetition': args.calls, 'us_per_call': us,
            'us_per_call_median': {n: {k: float(np.median(v)) for k, v in cols.items()} for n, cols in us.items()},
            'note': 'confusion covers all frames of the batch in one launch; boundary and distance_histogram one frame; Agreement.add = confusion + 8 launches per frame'}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
