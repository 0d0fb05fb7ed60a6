"""Time frame resampling on the GPU (pix2pix3d_amd/resample.py, csrc/video/frame_resample.hip) against what a user does without it, print ONE JSON
line and write it to --out.

The clip: --frames (120) frames of 512 x 512 RGB, the smooth gradients with three grey levels of noise of tests/video_cases.gradient_frames' formula,
made on the device; the index clip of the nearest leg is its red channel >> 4 (16 labels).  Four legs:
    512 -> 256 lanczos      512 -> 128 box      128 -> 512 bicubic (from the box leg's result)      512 -> 256 nearest on the index clip
and for each of them
    device_ms        resample.resize into a preallocated ``out=``: device events around --calls calls in a row, the median of --reps (tables cached)
    passes           per pass: the bytes it must read and write (source rows it reads + result, from the shapes) and, from a second window of
                     events around each entry point alone, its time and bytes / time
    host_pil_ms      (a) what a user does today: the clip to the host, ``PIL.Image.resize`` of every frame, the results back to the device (host clock
                     around work that ends in a synchronise, the median of --pil-reps); its bytes are checked against the device's: ``equal``
    interpolate_ms   (b) ``torch.nn.functional.interpolate(..., antialias=True)`` on the device in float32 with the round trip through float and back
                     (for scale only: its bytes differ — 'nearest' legs use mode='nearest'); ``interpolate_differs`` is the share of bytes that do
Usage: python tools/bench_resample.py [--frames 120] [--reps 5] [--calls 10] [--pil-reps 2] [--out profiles/resample_bench.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PIL_CODE = {'nearest': 0, 'lanczos': 1, 'bilinear': 2, 'bicubic': 3, 'box': 4, 'hamming': 5}      # PIL.Image.Resampling
INTERPOLATE_MODE = {'nearest': 'nearest', 'box': 'area', 'bilinear': 'bilinear', 'bicubic': 'bicubic', 'lanczos': 'bicubic', 'hamming': 'bilinear'}


def gradient_clip(f, h, w, dev):
    """tests/video_cases.gradient_frames, made on the device frame by frame."""
    y, x = torch.meshgrid(torch.arange(h, dtype=torch.float64, device=dev), torch.arange(w, dtype=torch.float64, device=dev), indexing='ij')
    gen = torch.Generator(device=dev).manual_seed(7)
    clip = torch.empty([f, h, w, 3], dtype=torch.uint8, device=dev)
    for i in range(f):
        t = 6.0 * (x + y) / (h + w) + 2 * np.pi / 120 * i
        rgb = torch.stack([127.5 + 127.5 * torch.sin(t), 127.5 + 127.5 * torch.sin(t + 2.0), 255 * y / (h - 1)], dim=2)
        clip[i] = (rgb + torch.randint(-3, 4, rgb.shape, device=dev, generator=gen)).clamp(0, 255).to(torch.uint8)
    return clip


def event_ms(fn, calls, reps):
    """The median over ``reps`` of the device time of one call, from events around ``calls`` calls in a row."""
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for _ in range(calls):
            fn()
        end.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(end) / calls)
    return statistics.median(times)


def host_ms(fn, reps):
    times = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(times), out


def pil_round_trip(clip, size, filter):
    from PIL import Image
    host = clip.cpu().numpy()
    out = np.stack([np.asarray(Image.fromarray(frame).resize(size, PIL_CODE[filter])) for frame in host])
    return torch.from_numpy(out).to(clip.device)


def interpolate(clip, size, filter):
    x = (clip if clip.ndim == 4 else clip[..., None]).permute(0, 3, 1, 2).float()
    mode = INTERPOLATE_MODE[filter]
    if mode == 'nearest':
        y = torch.nn.functional.interpolate(x, size=(size[1], size[0]), mode='nearest')
    elif mode == 'area':
        y = torch.nn.functional.interpolate(x, size=(size[1], size[0]), mode='area')
    else:
        y = torch.nn.functional.interpolate(x, size=(size[1], size[0]), mode=mode, antialias=True, align_corners=False)
    y = (y + 0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1)
    return y.contiguous() if clip.ndim == 4 else y[..., 0].contiguous()


def passes(clip, size, filter, calls, reps):
    """Per pass of ``resize(clip, size, filter)``: what it must move and how long the entry point alone takes."""
    from pix2pix3d_amd import resample
    f, h, w = clip.shape[:3]
    bpp = clip.shape[3] if clip.ndim == 4 else 1
    ow, oh = size
    dev, rest = clip.device, list(clip.shape[3:])
    rows = []
    if filter == 'nearest':
        (xi,), (yi,) = resample._tables(w, ow, 'nearest', None, dev), resample._tables(h, oh, 'nearest', None, dev)
        out = torch.empty([f, oh, ow] + rest, dtype=torch.uint8, device=dev)
        ms = event_ms(lambda: resample._nearest(clip, xi, yi, out), calls, reps)
        rows.append(('nearest', 2 * f * oh * ow * bpp, ms))                      # every output byte is read once and written once
    else:
        by, ky, first, last = resample._tables(h, oh, filter, None, dev, shifted=True)
        bx, kx = resample._tables(w, ow, filter, None, dev)[:2]
        src = clip[:, first:last]
        mid = torch.empty([f, last - first, ow] + rest, dtype=torch.uint8, device=dev)
        out = torch.empty([f, oh, ow] + rest, dtype=torch.uint8, device=dev)
        ms = event_ms(lambda: resample._pass_device(src, 2, bx, kx, mid), calls, reps)
        rows.append(('rows', f * (last - first) * (w + ow) * bpp, ms))
        ms = event_ms(lambda: resample._pass_device(mid, 1, by, ky, out), calls, reps)
        rows.append(('columns', f * ((last - first) + oh) * ow * bpp, ms))
    return [{'pass': name, 'bytes': int(b), 'ms': round(ms, 4), 'gb_per_s': round(b / ms / 1e6, 1)} for name, b, ms in rows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=120)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--calls', type=int, default=10)
    ap.add_argument('--pil-reps', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'resample_bench.json'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'bench_resample.py measures on the GPU'
    import PIL
    from pix2pix3d_amd import resample
    dev = torch.device('cuda')
    clip = gradient_clip(args.frames, 512, 512, dev)
    small = resample.resize(clip, (128, 128), 'box')
    index = (clip[..., 0] >> 4).contiguous()
    legs = (('512 -> 256 lanczos', clip, (256, 256), 'lanczos'), ('512 -> 128 box', clip, (128, 128), 'box'),
            ('128 -> 512 bicubic', small, (512, 512), 'bicubic'), ('512 -> 256 nearest (index clip)', index, (256, 256), 'nearest'))
    result = {'tool': 'bench_resample', 'device': torch.cuda.get_device_name(0), 'pillow': PIL.__version__, 'frames': args.frames, 'reps': args.reps,
              'calls': args.calls, 'pil_reps': args.pil_reps, 'legs': {}}
    for name, src, size, filter in legs:
        out = torch.empty([src.shape[0], size[1], size[0]] + list(src.shape[3:]), dtype=torch.uint8, device=dev)
        leg = {'device_ms': round(event_ms(lambda: resample.resize(src, size, filter, out=out), args.calls, args.reps), 4),
               'passes': passes(src, size, filter, args.calls, args.reps)}
        pil_ms, reference = host_ms(lambda: pil_round_trip(src, size, filter), args.pil_reps)
        leg['host_pil_ms'], leg['equal'] = round(pil_ms, 2), bool(torch.equal(reference, out))
        other = interpolate(src, size, filter)
        leg['interpolate_ms'] = round(event_ms(lambda: interpolate(src, size, filter), max(1, args.calls // 2), args.reps), 4)
        leg['interpolate_differs'] = round(float((other != out).float().mean()), 4)
        leg['speedup_over_host_pil'] = round(leg['host_pil_ms'] / leg['device_ms'], 1)
        result['legs'][name] = leg
    line = json.dumps(result)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(line + '\n')
    print(line)


if __name__ == '__main__':
    main()
