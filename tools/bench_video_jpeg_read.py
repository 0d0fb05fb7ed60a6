"""Reading a 120-frame Motion-JPEG clip of 512^2 frames back to device frames, two ways on the same box and the same file, at 4:2:0 and 4:4:4:

(a) the host loop the feature replaces: ``video.read_avi``, every frame decoded by PIL (libjpeg, one core), the frames stacked and uploaded in one copy;
(b) ``video.decode_avi(path, device='cuda')``: headers parsed on the host, the scans uploaded in one copy, entropy decoding (``p3d_video_jpeg_unscan``, a
    lane per restart interval), dequantiser, inverse DCT, chroma filter and colour transform on the device (libp3d_video.so).

The clip is tools/bench_video_jpeg.py's: synthetic and continuous-tone, written by ``video.save_avi`` at ``--quality`` (restart intervals of 8 MCUs: 128 or
512 lanes a frame).  The same two routes then read a Pillow-written set of the same frames WITHOUT restart markers (optimised tables): one interval, so one
lane, a frame — the case the docstring of ``jpeg_unscan`` calls correct but slow.  End to end: host clock around each call, which starts with the file on
disk (in the page cache) or the list of streams and ends with uint8 [F, H, W, 3] on the device, after a synchronise; one warm-up of each, then ``--reps``
repetitions of (b) and ``--pil-reps`` of (a), interleaved; medians.  The kernels: device events around the fill + launch of ``p3d_video_jpeg_unscan`` and
around the two launches of ``p3d_video_jpeg_decode`` (``_lib.kernel_timer``), medians.  How far the two routes' pixels lie apart is reported too.

    python tools/bench_video_jpeg_read.py [--frames 120] [--reps 9] [--pil-reps 3] [--quality 90] [--out profiles/video_jpeg_read_bench.json]

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
    ap.add_argument('--size', type=int, default=512)
    ap.add_argument('--reps', type=int, default=9)
    ap.add_argument('--pil-reps', type=int, default=3)
    ap.add_argument('--quality', type=int, default=90)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from PIL import Image
    from pix2pix3d_amd import _lib, video
    assert torch.cuda.is_available(), 'bench_video_jpeg_read.py measures the device kernels: it needs the GPU'
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

    def host_loop(streams):
        return torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(s)).convert('RGB')) for s in streams])).to(dev)

    kernels = ('video_jpeg_unscan', 'video_jpeg_decode')

    def measure(ours, theirs):
        """Medians of the two routes, the kernels' times inside ours, and how far the pixels lie apart."""
        _, a = seconds(ours)
        _, b = seconds(theirs)
        t_dev, t_pil = [], []
        for name in kernels:
            _lib.kernel_events[name] = []
        for rep in range(max(args.reps, args.pil_reps)):
            if rep < args.pil_reps:
                t_pil.append(seconds(theirs)[0])
            if rep < args.reps:
                t_dev.append(seconds(ours)[0])
        kernel_us = {name: [round(e0.elapsed_time(e1) * 1e3, 1) for e0, e1 in _lib.kernel_events.pop(name)] for name in kernels}
        d = (a.to(torch.int16) - b.to(torch.int16)).abs()
        return {'device_s': [round(t, 4) for t in t_dev], 'host_loop_s': [round(t, 4) for t in t_pil], 'device_s_median': float(np.median(t_dev)),
                'host_loop_s_median': float(np.median(t_pil)), 'speedup_median': round(float(np.median(t_pil) / np.median(t_dev)), 2), 'kernel_us': kernel_us,
                'kernel_us_median': {k: float(np.median(v)) for k, v in kernel_us.items()}, 'largest_difference_levels': int(d.max()),
                'pixels_that_differ': round(float((d > 0).float().mean()), 5)}

    tmp = tempfile.mkdtemp()
    frames = gradient_clip(args.frames, args.size, args.size)
    results = {}
    for subsampling in ('4:2:0', '4:4:4'):
        path = os.path.join(tmp, f'clip{subsampling[-1]}.avi')
        video.save_avi(path, frames, quality=args.quality, subsampling=subsampling)
        r = measure(lambda: video.decode_avi(path, device=dev)[0], lambda: host_loop(video.read_avi(path)[0]))
        r['exact'] = bool(torch.equal(video.decode_avi(path, device=dev)[0], video.jpeg_reconstruct(frames, args.quality, subsampling)))
        r['file_bytes'], r['intervals_a_frame'] = os.path.getsize(path), video.jpeg_layout(args.size, args.size, subsampling)[3]
        results[f'save_avi {subsampling}'] = r
        streams = []
        for a in frames.cpu().numpy():
            out = io.BytesIO()
            Image.fromarray(a).save(out, 'JPEG', quality=args.quality, subsampling={'4:4:4': 0, '4:2:0': 2}[subsampling], optimize=True)
            streams.append(out.getvalue())
        r = measure(lambda: video.decode_jpeg(streams, device=dev), lambda: host_loop(streams))
        r['file_bytes'], r['intervals_a_frame'] = sum(map(len, streams)), 1
        results[f'Pillow, no restart markers {subsampling}'] = r

    for name, r in results.items():
        print(f'{name}: {args.frames} frames of {args.size} x {args.size}, quality {args.quality}, {r["file_bytes"]} bytes, {r["intervals_a_frame"]} intervals a frame')
        print(f'  {"host loop (PIL decode, stack, upload), s, median":50s}{r["host_loop_s_median"]:10.4f}')
        print(f'  {"device route, s, median":50s}{r["device_s_median"]:10.4f}   ({r["speedup_median"]}x)   pixels apart: at most {r["largest_difference_levels"]} levels, '
              f'{100 * r["pixels_that_differ"]:.2f}% differ')
        for k, v in r['kernel_us_median'].items():
            print(f'  {k:50s}{v:10.1f} us')
    line = {'workload': f'{args.frames} synthetic continuous-tone frames (travelling colour gradients, three grey levels of noise) at {args.size} x {args.size}, quality '
                        f'{args.quality}: a save_avi file, and Pillow streams without restart markers (optimize=True); the file or the streams in, device frames out',
            'device': torch.cuda.get_device_name(0), 'host_cpus_used_by_the_host_loop': 1, 'restart_interval_mcus': video.JPEG_RESTART, 'results': results,
            'note': 'host_loop = PIL.Image.open(...).convert("RGB") per frame, np.stack, one upload; device route = decode_avi / decode_jpeg; kernel_us are device '
                    'events around the fill + launch of jpeg_unscan and the two launches of jpeg_decode inside the timed calls'}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
