"""Encoding a 120-frame clip as baseline JPEGs, two ways on the same box and the same device frames, at 512^2 and at 128^2:

(a) the host loop the feature replaces: the frames copied to the host and every frame saved by PIL (libjpeg, one core) at the same quality and subsampling —
    the same quantisation and Huffman tables; the copy is part of the time;
(b) ``video.encode_jpeg``: colour transform, DCT, quantiser and entropy coder on the device (libp3d_video.so), only the scans copied.

The clip is synthetic and continuous-tone — tests/video_cases.gradient_frames' formula made on the device: travelling colour gradients with three grey levels
of noise, what a trained generator's frames are to an encoder (a random-weight generator paints nearly flat frames, which flatter both routes).  End to end:
host clock around each call, which starts with device frames and ends with the list of streams on the host, after a synchronise; one warm-up of each, then
``--reps`` repetitions of (b) and ``--pil-reps`` of (a), interleaved; medians.  ``video.save_avi`` is timed the same way (it ends with the file written).  The
kernels: device events around the one ``p3d_video_jpeg_blocks`` launch and around each of the two ``p3d_video_jpeg_scan`` launches of every repetition of (b)
(``_lib.kernel_timer``), medians.  Both routes' bytes, and the PSNR of both routes' decoded frames against the source over eight frames of the clip.

    python tools/bench_video_jpeg.py [--frames 120] [--reps 9] [--pil-reps 3] [--quality 90] [--subsampling 4:2:0] [--out profiles/video_jpeg_bench.json]

Prints a table and ONE JSON line."""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=120)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--pil-reps', type=int, default=3)
    ap.add_argument('--quality', type=int, default=90)
    ap.add_argument('--subsampling', default='4:2:0', choices=['4:4:4', '4:2:0'])
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from PIL import Image
    from pix2pix3d_amd import _lib, video
    assert torch.cuda.is_available(), 'bench_video_jpeg.py measures the device kernels: it needs the GPU'
    dev = torch.device('cuda')
    pil_subsampling = {'4:4:4': 0, '4:2:0': 2}[args.subsampling]

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

    def host_loop(frames):
        streams = []
        for a in frames.cpu().numpy():
            out = io.BytesIO()
            Image.fromarray(a).save(out, 'JPEG', quality=args.quality, subsampling=pil_subsampling)
            streams.append(out.getvalue())
        return streams

    def decoded(streams, which):
        return np.stack([np.asarray(Image.open(io.BytesIO(streams[i])).convert('RGB')) for i in which])

    def psnr(a, b):
        return float(10 * np.log10(255.0 ** 2 / ((a.astype(np.float64) - b.astype(np.float64)) ** 2).mean()))

    tmp = tempfile.mkdtemp()
    kernels = ('video_jpeg_blocks', 'video_jpeg_scan_lengths', 'video_jpeg_scan_bytes')
    results = {}
    for size in (512, 128):
        frames = gradient_clip(args.frames, size, size)
        device_route = lambda: video.encode_jpeg(frames, args.quality, args.subsampling)
        _, ours = seconds(device_route)                                            # warm-up: code objects, the constant tables, allocation sizes
        _, pils = seconds(lambda: host_loop(frames))
        seconds(lambda: video.save_avi(os.path.join(tmp, 'clip.avi'), frames, quality=args.quality, subsampling=args.subsampling))
        t_dev, t_pil, t_avi = [], [], []
        for name in kernels:
            _lib.kernel_events[name] = []
        for rep in range(max(args.reps, args.pil_reps)):
            if rep < args.pil_reps:
                t_pil.append(seconds(lambda: host_loop(frames))[0])
            if rep < args.reps:
                t_dev.append(seconds(device_route)[0])
        kernel_us = {name: [round(e0.elapsed_time(e1) * 1e3, 1) for e0, e1 in _lib.kernel_events.pop(name)] for name in kernels}
        for rep in range(min(args.reps, 3)):
            t_avi.append(seconds(lambda: video.save_avi(os.path.join(tmp, 'clip.avi'), frames, quality=args.quality, subsampling=args.subsampling))[0])
        which = list(range(0, args.frames, max(1, args.frames // 8)))[:8]
        source = frames[which].cpu().numpy()
        results[f'{size}x{size}'] = {
            'frames': args.frames, 'raw_bytes': int(frames.numel()),
            'encode_jpeg_s': [round(t, 4) for t in t_dev], 'host_loop_s': [round(t, 4) for t in t_pil], 'save_avi_s': [round(t, 4) for t in t_avi],
            'encode_jpeg_s_median': float(np.median(t_dev)), 'host_loop_s_median': float(np.median(t_pil)), 'save_avi_s_median': float(np.median(t_avi)),
            'speedup_median': round(float(np.median(t_pil) / np.median(t_dev)), 2),
            'kernel_us': kernel_us, 'kernel_us_median': {k: float(np.median(v)) for k, v in kernel_us.items()},
            'bytes': {'encode_jpeg': sum(map(len, ours)), 'host_loop': sum(map(len, pils)), 'avi_file': os.path.getsize(os.path.join(tmp, 'clip.avi'))},
            'psnr_db': {'encode_jpeg': round(psnr(decoded(ours, which), source), 2), 'host_loop': round(psnr(decoded(pils, which), source), 2)}}

    for name, r in results.items():
        print(f'{name}, {r["frames"]} frames, quality {args.quality}, {args.subsampling}')
        print(f'  {"host loop (copy + PIL), s, median":50s}{r["host_loop_s_median"]:10.4f}   {r["bytes"]["host_loop"]:10d} bytes, {r["psnr_db"]["host_loop"]} dB')
        print(f'  {"video.encode_jpeg, s, median":50s}{r["encode_jpeg_s_median"]:10.4f}   {r["bytes"]["encode_jpeg"]:10d} bytes, {r["psnr_db"]["encode_jpeg"]} dB'
              f'   ({r["speedup_median"]}x)')
        print(f'  {"video.save_avi, s, median":50s}{r["save_avi_s_median"]:10.4f}   {r["bytes"]["avi_file"]:10d} bytes')
        for k, v in r['kernel_us_median'].items():
            print(f'  {k:50s}{v:10.1f} us')
    line = {'workload': f'{args.frames} synthetic continuous-tone frames (travelling colour gradients, three grey levels of noise) at 512 x 512 and 128 x 128, '
                        f'quality {args.quality}, {args.subsampling}; device frames in, the list of JPEG streams on the host out',
            'device': torch.cuda.get_device_name(0), 'host_cpus_used_by_the_host_loop': 1, 'restart_interval_mcus': video.JPEG_RESTART, 'results': results,
            'note': 'host_loop = frames.cpu() and PIL.Image.save(quality, subsampling) per frame into memory: the same quantisation and Huffman tables; kernel_us '
                    'are device events around single launches inside the timed encode_jpeg calls (the event pair is on only during this measurement)'}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
