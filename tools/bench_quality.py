"""Judging a JPEG setting on a 120-frame clip of 512 x 512, three ways on the same box and the same device frames:

(ours) ``video.jpeg_reconstruct`` (what a decoder shows, made where the frames are: three launches) and ``quality.compare`` of it against the frames (the
       error sums and SSIM: two launches and one host read);
(a)    the torch formulation of ``compare`` on the device — the definition the kernels equal, int64 tensors and fp64 divisions, eight frames at a time (its
       temporaries are 40 times the clip);
(b)    the host loop both replace: the frames copied to the host, every frame's stream (``video.encode_jpeg``'s, made beforehand and not timed) decoded by PIL
       on one core, then MSE and the textbook fp64 SSIM in numpy, frame by frame.

The clip is synthetic and continuous-tone — tests/video_cases.gradient_frames' formula made on the device, as tools/bench_video_jpeg.py makes it: a
random-weight generator paints nearly flat frames, which flatter every route.  Host clock around each call, from device frames to the metrics on the host,
after a synchronise; one warm-up of each, then ``--reps`` repetitions of ours and ``--slow-reps`` of (a) and (b); medians.  The kernels: device events around
the single launches inside the timed calls (``_lib.kernel_timer``), medians.  ``video.jpeg_quality_for`` (seven steps on eight frames) is timed the same way.

    python tools/bench_quality.py [--frames 120] [--size 512] [--reps 9] [--slow-reps 2] [--quality 90] [--subsampling 4:2:0] [--out profiles/quality_bench.json]

Prints a table and ONE JSON line."""
import argparse
import io
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
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--slow-reps', type=int, default=2)
    ap.add_argument('--quality', type=int, default=90)
    ap.add_argument('--subsampling', default='4:2:0', choices=['4:4:4', '4:2:0'])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from PIL import Image
    from pix2pix3d_amd import _lib, quality as Q, video
    assert torch.cuda.is_available(), 'bench_quality.py measures the device kernels: it needs the GPU'
    dev = torch.device('cuda')

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
    shown = video.jpeg_reconstruct(frames, args.quality, args.subsampling)
    streams = video.encode_jpeg(frames, args.quality, args.subsampling)
    f, h, w = frames.shape[:3]

    def torch_route():
        error = torch.zeros([f, 3, 4], dtype=torch.int64, device=dev)
        ssim = torch.zeros([f, 3, 2], dtype=torch.int64, device=dev)
        for i in range(0, f, 8):
            Q._error_sums_torch(shown[i:i + 8], frames[i:i + 8], error[i:i + 8])
            Q._ssim_torch(shown[i:i + 8], frames[i:i + 8], ssim[i:i + 8], False)
        return Q.metrics_from_sums(error, ssim, samples=h * w)

    g = np.exp(-((np.arange(11) - 5.0) ** 2) / 4.5)
    g /= g.sum()

    def numpy_ssim(a, b):
        def blur(q):
            rows = sum(g[k] * q[:, k:k + w - 10] for k in range(11))
            return sum(g[k] * rows[k:k + h - 10] for k in range(11))
        mx, my = blur(a), blur(b)
        vx, vy, cxy = blur(a * a) - mx * mx, blur(b * b) - my * my, blur(a * b) - mx * my
        return float((((2 * mx * my + 6.5025) * (2 * cxy + 58.5225)) / ((mx * mx + my * my + 6.5025) * (vx + vy + 58.5225))).mean())

    host_times = {}

    def host_route():
        t0 = time.perf_counter()
        source = frames.cpu().numpy()
        t1 = time.perf_counter()
        decoded = [np.asarray(Image.open(io.BytesIO(s)).convert('RGB')) for s in streams]
        t2 = time.perf_counter()
        mse, ssim = [], []
        for a, b in zip(decoded, source):
            a, b = a.astype(np.float64), b.astype(np.float64)
            mse.append(((a - b) ** 2).mean())
            ssim.append(numpy_ssim(a, b))
        t3 = time.perf_counter()
        host_times.setdefault('copy_s', []).append(t1 - t0)
        host_times.setdefault('pil_decode_s', []).append(t2 - t1)
        host_times.setdefault('numpy_metrics_s', []).append(t3 - t2)
        return {'psnr': float(10 * np.log10(255.0 ** 2 / np.mean(mse))), 'ssim': float(np.mean(ssim))}

    kernels = ('video_jpeg_blocks', 'video_jpeg_decode', 'video_error_sums', 'video_ssim')
    _, ours = seconds(lambda: Q.compare(shown, frames))                             # warm-ups
    seconds(lambda: video.jpeg_reconstruct(frames, args.quality, args.subsampling))
    _, by_torch = seconds(torch_route)
    _, by_host = seconds(host_route)
    host_times.clear()
    seconds(lambda: video.jpeg_quality_for(frames, ssim=0.95, subsampling=args.subsampling))
    for name in kernels:
        _lib.kernel_events[name] = []
    t_compare = [seconds(lambda: Q.compare(shown, frames))[0] for _ in range(args.reps)]
    t_reconstruct = [seconds(lambda: video.jpeg_reconstruct(frames, args.quality, args.subsampling))[0] for _ in range(args.reps)]
    kernel_us = {name: [round(e0.elapsed_time(e1) * 1e3, 1) for e0, e1 in _lib.kernel_events.pop(name)] for name in kernels}
    t_search = [seconds(lambda: video.jpeg_quality_for(frames, ssim=0.95, subsampling=args.subsampling)) for _ in range(min(args.reps, 3))]
    t_torch = [seconds(torch_route)[0] for _ in range(args.slow_reps)]
    t_host = [seconds(host_route)[0] for _ in range(args.slow_reps)]

    med = lambda v: float(np.median(v))
    result = {'frames': f, 'size': [h, w], 'quality': args.quality, 'subsampling': args.subsampling,
              'compare_s': [round(t, 5) for t in t_compare], 'jpeg_reconstruct_s': [round(t, 5) for t in t_reconstruct],
              'torch_formulation_s': [round(t, 4) for t in t_torch], 'host_loop_s': [round(t, 4) for t in t_host],
              'host_loop_parts_s_median': {k: round(med(v), 4) for k, v in host_times.items()},
              'jpeg_quality_for_s': [round(t, 4) for t, _ in t_search], 'jpeg_quality_for_result': [t_search[0][1][0], t_search[0][1][2]],
              'compare_s_median': med(t_compare), 'jpeg_reconstruct_s_median': med(t_reconstruct), 'torch_formulation_s_median': med(t_torch),
              'host_loop_s_median': med(t_host), 'jpeg_quality_for_s_median': med([t for t, _ in t_search]),
              'kernel_us_median': {k: med(v) for k, v in kernel_us.items()},
              'metrics': {'kernels': {k: ours[k] for k in ('psnr', 'ssim')}, 'host_loop': by_host}, 'torch_formulation_equals_kernels': by_torch == ours}
    print(f'{f} frames of {h} x {w}, quality {args.quality}, {args.subsampling}')
    for label, key in (('quality.compare, s, median', 'compare_s_median'), ('video.jpeg_reconstruct, s, median', 'jpeg_reconstruct_s_median'),
                       ('(a) torch formulation of compare on the device, s', 'torch_formulation_s_median'),
                       ('(b) copy + PIL decode + numpy metrics, s', 'host_loop_s_median'), ('video.jpeg_quality_for (8 frames), s', 'jpeg_quality_for_s_median')):
        print(f'  {label:56s}{result[key]:10.4f}')
    for k, v in result['kernel_us_median'].items():
        print(f'  {k:56s}{v:10.1f} us')
    line = {'workload': f'{f} synthetic continuous-tone frames (travelling colour gradients, three grey levels of noise) at {h} x {w} against their JPEG '
                        f'reconstruction at quality {args.quality}, {args.subsampling}; device frames in, the metrics dict on the host out',
            'device': torch.cuda.get_device_name(0), 'host_cpus_used_by_the_host_loop': 1, 'result': result,
            'note': 'host_loop decodes streams made beforehand (not timed) with PIL and computes MSE and a textbook fp64 SSIM in numpy per frame; its PSNR and '
                    'SSIM differ from the kernels\' by the decoders\' rounding and the 10-bit window; kernel_us are device events around single launches inside '
                    'the timed calls'}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
