"""MS-SSIM of a 120-frame clip of 512 x 512 RGB against its JPEG reconstruction, four ways on the same box and the same device frames:

(fused)  ``multiscale.ms_ssim``: five launches of ``p3d_frame_msssim_level``, each of which also writes the next level of both clips, and one host read;
(split)  the same with ``fused=False``: ``p3d_frame_halve`` for each clip and level (eight launches) and the level kernel only measuring (five);
(a)      the torch formulation on the device — the definition the kernels equal, int64 tensors and fp64 divisions, eight frames at a time;
(b)      the host route both replace: both clips copied to the host, then the textbook float64 formulation in numpy on one core, frame by frame.

The clip is tools/bench_quality.py's (travelling colour gradients with three grey levels of noise, made on the device).  Host clock around each call, from
device frames to the metrics on the host, after a synchronise; one warm-up of each, then ``--reps`` rounds that ALTERNATE fused and split, and
``--slow-reps`` of (a) and (b); medians.  The kernels: device events around the single launches inside the timed calls (``_lib.kernel_timer``), medians
per level — the fused launches in the fused rounds, the measuring launches and the halvings in the split rounds.

    python tools/bench_multiscale.py [--frames 120] [--size 512] [--reps 15] [--slow-reps 2] [--quality 75] [--out profiles/multiscale_bench.json]

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=120)
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=15)
    ap.add_argument('--slow-reps', type=int, default=2)
    ap.add_argument('--quality', type=int, default=75)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'multiscale_bench.json'))
    args = ap.parse_args()
    from pix2pix3d_amd import _lib, multiscale as M, video
    assert torch.cuda.is_available(), 'bench_multiscale.py measures the device kernels: it needs the GPU'
    dev = torch.device('cuda')
    levels = M.MAX_LEVELS

    def gradient_clip(f, h, w):
        y, x = torch.meshgrid(torch.arange(h, dtype=torch.float64, device=dev), torch.arange(w, dtype=torch.float64, device=dev), indexing='ij')
        gen = torch.Generator(device=dev).manual_seed(7)
        clip = torch.empty([f, h, w, 3], dtype=torch.uint8, device=dev)
        for i in range(f):
            t = 6.0 * (x + y) / (h + w) + 2 * np.pi / 120 * i
            rgb = torch.stack([127.5 + 127.5 * torch.sin(t), 127.5 + 127.5 * torch.sin(t + 2.0), 255 * y / (h - 1)], dim=2)
            clip[i] = (rgb + torch.randint(-3, 4, rgb.shape, device=dev, generator=gen)).clamp(0, 255).to(torch.uint8)
        return clip

    def seconds(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    frames = gradient_clip(args.frames, args.size, args.size)
    shown = video.jpeg_reconstruct(frames, args.quality, '4:2:0')
    f, h, w = frames.shape[:3]

    def torch_route():
        sums = torch.zeros([f, 3, levels, 3], dtype=torch.int64, device=dev)
        for i in range(0, f, 8):
            a, b = shown[i:i + 8], frames[i:i + 8]
            for k in range(levels):
                M._level_torch(a, b, sums[i:i + 8, :, k])
                if k + 1 < levels:
                    a, b = M._halve_torch(a), M._halve_torch(b)
        return M.metrics_from_msssim(sums)

    g = np.exp(-((np.arange(11) - 5.0) ** 2) / 4.5)
    g /= g.sum()
    weights = M.default_weights(levels)

    def numpy_msssim(a, b):
        """One frame [H, W, 3], float64: the textbook formulation, unrounded 2 x 2 mean pooling; the mean over the channels."""
        result = np.ones(3)
        for k in range(levels):
            hh, ww = a.shape[:2]

            def blur(q):
                rows = sum(g[t] * q[:, t:t + ww - 10] for t in range(11))
                return sum(g[t] * rows[t:t + hh - 10] for t in range(11))
            mx, my = blur(a), blur(b)
            vx, vy, cxy = blur(a * a) - mx * mx, blur(b * b) - my * my, blur(a * b) - mx * my
            term = (2 * cxy + 58.5225) / (vx + vy + 58.5225)
            if k + 1 == levels:
                term = term * (2 * mx * my + 6.5025) / (mx * mx + my * my + 6.5025)
            result = result * np.maximum(term.mean(axis=(0, 1)), 0.0) ** weights[k]
            if k + 1 < levels:
                a, b = (0.25 * (t[0:hh // 2 * 2:2, 0:ww // 2 * 2:2] + t[0:hh // 2 * 2:2, 1:ww // 2 * 2:2] + t[1:hh // 2 * 2:2, 0:ww // 2 * 2:2]
                                + t[1:hh // 2 * 2:2, 1:ww // 2 * 2:2]) for t in (a, b))
        return float(result.mean())

    host_times = {}

    def host_route():
        t0 = time.perf_counter()
        a, b = shown.cpu().numpy(), frames.cpu().numpy()
        t1 = time.perf_counter()
        values = [numpy_msssim(x.astype(np.float64), y.astype(np.float64)) for x, y in zip(a, b)]
        t2 = time.perf_counter()
        host_times.setdefault('copy_s', []).append(t1 - t0)
        host_times.setdefault('numpy_s', []).append(t2 - t1)
        return {'ms_ssim': float(np.mean(values))}

    fused_route = lambda: M.metrics_from_msssim(M.msssim_sums(shown, frames, levels, fused=True))
    split_route = lambda: M.metrics_from_msssim(M.msssim_sums(shown, frames, levels, fused=False))
    _, by_fused = seconds(fused_route)                                             # warm-ups
    _, by_split = seconds(split_route)
    _, by_torch = seconds(torch_route)
    _, by_host = seconds(host_route)
    host_times.clear()
    kernels = [f'frame_msssim_level{k}' for k in range(levels)] + ['frame_halve']
    t_fused, t_split, fused_us, split_us = [], [], {k: [] for k in kernels[:-1]}, {k: [] for k in kernels}
    for _ in range(args.reps):                                                      # alternating: the two routes see the same box
        for route, times, log in ((fused_route, t_fused, fused_us), (split_route, t_split, split_us)):
            for name in log:
                _lib.kernel_events[name] = []
            times.append(seconds(route)[0])
            for name in log:
                log[name] += [e0.elapsed_time(e1) * 1e3 for e0, e1 in _lib.kernel_events.pop(name)]
    t_torch = [seconds(torch_route)[0] for _ in range(args.slow_reps)]
    t_host = [seconds(host_route)[0] for _ in range(args.slow_reps)]

    med = lambda v: float(np.median(v))
    halvings = np.asarray(split_us['frame_halve']).reshape(args.reps, levels - 1, 2).sum(axis=2)      # per round and level: both clips
    result = {'frames': f, 'size': [h, w], 'levels': levels, 'quality': args.quality, 'reps': args.reps,
              'fused_s': [round(t, 5) for t in t_fused], 'split_s': [round(t, 5) for t in t_split],
              'torch_formulation_s': [round(t, 4) for t in t_torch], 'host_route_s': [round(t, 4) for t in t_host],
              'host_route_parts_s_median': {k: round(med(v), 4) for k, v in host_times.items()},
              'fused_s_median': med(t_fused), 'split_s_median': med(t_split), 'torch_formulation_s_median': med(t_torch), 'host_route_s_median': med(t_host),
              'fused_s_min_max': [min(t_fused), max(t_fused)], 'split_s_min_max': [min(t_split), max(t_split)],
              'fused_level_us_median': [round(med(fused_us[k]), 1) for k in kernels[:-1]],
              'split_level_us_median': [round(med(split_us[k]), 1) for k in kernels[:-1]],
              'split_halve_both_clips_us_median': [round(med(halvings[:, k]), 1) for k in range(levels - 1)],
              'metrics': {'kernels': by_fused['ms_ssim'], 'level_cs': by_fused['level_cs'], 'level_q': by_fused['level_q'], 'host_route': by_host['ms_ssim']},
              'split_equals_fused': by_split == by_fused, 'torch_formulation_equals_kernels': by_torch == by_fused}
    result['fused_kernels_us_median'] = round(sum(result['fused_level_us_median']), 1)
    result['split_kernels_us_median'] = round(sum(result['split_level_us_median']) + sum(result['split_halve_both_clips_us_median']), 1)
    print(f'{f} frames of {h} x {w} RGB against their JPEG reconstruction at quality {args.quality}, {levels} levels')
    for label, key in (('multiscale.ms_ssim fused, s, median', 'fused_s_median'), ('multiscale.ms_ssim fused=False, s, median', 'split_s_median'),
                       ('(a) torch formulation on the device, s', 'torch_formulation_s_median'), ('(b) copy + float64 numpy, s', 'host_route_s_median')):
        print(f'  {label:56s}{result[key]:10.5f}')
    for k in range(levels):
        halve = f'{result["split_halve_both_clips_us_median"][k]:10.1f}' if k + 1 < levels else '         -'
        print(f'  level {k}: fused launch {result["fused_level_us_median"][k]:10.1f} us   measuring launch {result["split_level_us_median"][k]:10.1f} us   '
              f'two halvings {halve} us')
    line = {'workload': f'{f} synthetic continuous-tone frames (travelling colour gradients, three grey levels of noise) at {h} x {w} RGB against their JPEG '
                        f'reconstruction at quality {args.quality}, 4:2:0; device frames in, the MS-SSIM dict on the host out',
            'device': torch.cuda.get_device_name(0), 'host_cpus_used_by_the_host_route': 1, 'result': result,
            'note': 'fused and split alternate round by round; *_level_us and the halvings are device events around single launches inside the timed calls; '
                    'the host route computes the textbook float64 formulation (exact Gaussian, unrounded pooling), whose value differs from the kernels\' by '
                    'the integer rules'}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
