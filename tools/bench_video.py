"""Writing a 120-frame 512^2 video, two ways on the same box and the same frames (``views.render_views`` of seg2cat at bench size, random weights as in
bench.py, frames left on the device):

(a) ``mesh.save_gif``: the frames copied to the host, PIL quantising every frame to a palette of its own and LZW-coding it;
(b) ``video.save_gif``: one palette for the clip and the index frames made on the device (libp3d_video.so), PIL only LZW-coding 'P' images.

End to end: host clock around each call, which ends with the file written; ``--reps`` repetitions of (b) and ``--pil-reps`` of (a), interleaved, after one
warm-up of (b).  The stages of (b) are timed the same way, each ending in a device synchronise.  The three entry points alone: device events around
``--calls`` back-to-back calls after a warm-up, median and best of ``--reps`` (an entry point is all its launches: the histogram and the box sums zero their
result first).  The histogram is also timed on frames that stress its LDS adds differently — one colour (every add on one bin), a smooth gradient (long runs
of one bin inside a wave) and uniform noise (no runs) — since it merges a wave's runs of equal bins before adding.  Both files' sizes, and the PSNR of both
decoded files against the RGB frames (and of the device route without dither: the ordered dither trades PSNR for the absence of banding).  The random-weight
generator paints nearly flat frames of a few hundred colours, which PIL quantises quickly and almost losslessly; so the end-to-end pair is repeated once
on a synthetic clip of the same size made of smooth colour gradients with three grey levels of noise (tests/video_cases.gradient_frames' formula on the
device), which is what a trained generator's frames are to a quantiser.

    python tools/bench_video.py [--frames 120] [--reps 5] [--pil-reps 2] [--calls 20] [--out profiles/video_bench.json]

Prints a table and ONE JSON line."""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=120)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--pil-reps', type=int, default=2)
    ap.add_argument('--calls', type=int, default=20)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from bench_views import build
    from video_cases import decode_gif, psnr
    from pix2pix3d_amd import mesh, video, views
    assert torch.cuda.is_available(), 'bench_video.py measures the device kernels: it needs the GPU'
    dev = torch.device('cuda')
    G = build(dev)
    ws = torch.randn(1, G.backbone.num_ws, 512, generator=torch.Generator().manual_seed(1234)).to(dev)
    cams = views.video_cameras(G, 'seg2cat', args.frames).to(dev)
    frames = views.render_views(G, ws, cams, views_per_step=4, neural_rendering_resolution=128, noise_mode='const')['image']
    f, h, w = frames.shape[:3]
    tmp = tempfile.mkdtemp()
    path_pil, path_dev = os.path.join(tmp, 'pil.gif'), os.path.join(tmp, 'device.gif')

    def seconds(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    # ---- end to end, interleaved -----------------------------------------------------------------------------------------------------------
    seconds(lambda: video.save_gif(path_dev, frames))                            # warm-up: code objects, allocation sizes
    end_to_end = {'mesh.save_gif': [], 'video.save_gif': []}
    for rep in range(max(args.reps, args.pil_reps)):
        if rep < args.pil_reps:
            end_to_end['mesh.save_gif'].append(round(seconds(lambda: mesh.save_gif(path_pil, frames))[0], 3))
        if rep < args.reps:
            end_to_end['video.save_gif'].append(round(seconds(lambda: video.save_gif(path_dev, frames))[0], 3))

    def gradient_clip():
        """tests/video_cases.gradient_frames, made on the device frame by frame."""
        y, x = torch.meshgrid(torch.arange(h, dtype=torch.float64, device=dev), torch.arange(w, dtype=torch.float64, device=dev), indexing='ij')
        gen = torch.Generator(device=dev).manual_seed(7)
        clip = torch.empty_like(frames)
        for i in range(f):
            t = 6.0 * (x + y) / (h + w) + 2 * np.pi / 120 * i
            rgb = torch.stack([127.5 + 127.5 * torch.sin(t), 127.5 + 127.5 * torch.sin(t + 2.0), 255 * y / (h - 1)], dim=2)
            clip[i] = (rgb + torch.randint(-3, 4, rgb.shape, device=dev, generator=gen)).clamp(0, 255).to(torch.uint8)
        return clip
    smooth = gradient_clip()
    path_pil_s, path_dev_s = os.path.join(tmp, 'pil_smooth.gif'), os.path.join(tmp, 'device_smooth.gif')
    end_to_end_smooth = {'mesh.save_gif': [round(seconds(lambda: mesh.save_gif(path_pil_s, smooth))[0], 3)],
                         'video.save_gif': [round(seconds(lambda: video.save_gif(path_dev_s, smooth))[0], 3) for _ in range(2)]}

    # ---- the stages of (b) -------------------------------------------------------------------------------------------------------------------
    stages = {}
    for rep in range(args.reps):
        t, counts = seconds(lambda: video.histogram(frames).cpu())
        stages.setdefault('histogram and its copy to the host', []).append(t)
        t, (boxes, box_of) = seconds(lambda: video.median_cut(counts))
        stages.setdefault('median cut (host)', []).append(t)
        t, pal = seconds(lambda: video.palette_from_sums(video.box_sums(frames, box_of.to(dev))))
        stages.setdefault('lookup to the device, box sums, palette', []).append(t)
        t, indices = seconds(lambda: video.quantize(frames, pal, boxes.shape[0], 16))
        stages.setdefault('quantize', []).append(t)
        t, host = seconds(lambda: (indices.cpu(), pal.cpu()))
        stages.setdefault('indices to the host', []).append(t)
        t, _ = seconds(lambda: video.save_gif_indexed(path_dev, *host))
        stages.setdefault("PIL: 'P' images, LZW, the file", []).append(t)
    stages = {k: [round(x, 4) for x in v] for k, v in stages.items()}

    # ---- the entry points alone: device events -------------------------------------------------------------------------------------------------
    counts = video.histogram(frames).cpu()
    boxes, box_of = video.median_cut(counts)
    lookup = box_of.to(dev)
    pal = video.palette_from_sums(video.box_sums(frames, lookup))
    n_colors = torch.tensor([boxes.shape[0]], dtype=torch.int32, device=dev)
    out = torch.empty([f, h, w], dtype=torch.uint8, device=dev)
    flat = torch.empty_like(frames)
    flat[:] = torch.tensor([201, 17, 94], dtype=torch.uint8, device=dev)
    noise = torch.randint(0, 256, frames.shape, dtype=torch.uint8, device=dev)
    launches = {
        'histogram': lambda: video.histogram(frames),
        'box_sums': lambda: video.box_sums(frames, lookup),
        'quantize (dither 16)': lambda: video.quantize(frames, pal, n_colors, 16, out=out),
        'quantize (no dither)': lambda: video.quantize(frames, pal, n_colors, 0, out=out),
        'histogram, one colour': lambda: video.histogram(flat),
        'histogram, smooth gradient': lambda: video.histogram(smooth),
        'histogram, uniform noise': lambda: video.histogram(noise),
        'box_sums, one colour': lambda: video.box_sums(flat, lookup),
        'box_sums, smooth gradient': lambda: video.box_sums(smooth, lookup),
        'box_sums, uniform noise': lambda: video.box_sums(noise, lookup),
    }

    def event_us(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(args.calls):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / args.calls

    for fn in launches.values():
        event_us(fn)                                                             # warm-up
    us = {name: [] for name in launches}
    for rep in range(args.reps):                                                 # interleaved
        for name, fn in launches.items():
            us[name].append(round(event_us(fn), 1))

    # ---- sizes and quality -------------------------------------------------------------------------------------------------------------------
    def files(clip, paths):
        rgb, out = clip.cpu().numpy(), {}
        path_plain = os.path.join(tmp, 'device_no_dither.gif')
        video.save_gif(path_plain, clip, dither=0)
        for name, path in (('mesh.save_gif', paths[0]), ('video.save_gif', paths[1]), ('video.save_gif, dither 0', path_plain)):
            decoded = decode_gif(path)
            out[name] = {'bytes': os.path.getsize(path), 'frames_decoded': int(decoded.shape[0]),
                         'psnr_db': round(float(psnr(decoded, rgb)), 2) if decoded.shape == rgb.shape else None}
        return out
    video.save_gif(path_dev, frames)                                             # (the stage timing above wrote the same file last)
    quality, quality_smooth = files(frames, (path_pil, path_dev)), files(smooth, (path_pil_s, path_dev_s))
    n_rows = int(boxes.shape[0])
    pixels = f * h * w

    print(f'{"end to end, s (median, best)":44s}' + ''.join(f'{k:>26s}' for k in end_to_end))
    print(f'{"":44s}' + ''.join(f'{np.median(v):17.3f} {min(v):8.3f}' for v in end_to_end.values()))
    for name, v in stages.items():
        print(f'  {name:50s}{np.median(v) * 1e3:10.1f} ms')
    for name, v in us.items():
        print(f'  {name:50s}{np.median(v):10.1f} us (best {min(v):.1f})')
    for name, q in quality.items():
        print(f'  {name:50s}{q["bytes"]:12d} bytes, {q["psnr_db"]} dB, {q["frames_decoded"]} frames')
    print('smooth synthetic clip:', end_to_end_smooth)
    for name, q in quality_smooth.items():
        print(f'  {name:50s}{q["bytes"]:12d} bytes, {q["psnr_db"]} dB, {q["frames_decoded"]} frames')
    line = {'workload': f'{f} frames of {h} x {w} from views.render_views (seg2cat at bench size, random weights, seed 1234), fps 60, 256 colours, dither 16',
            'device': torch.cuda.get_device_name(0), 'end_to_end_s': end_to_end, 'end_to_end_s_median': {k: float(np.median(v)) for k, v in end_to_end.items()},
            'speedup_median': round(float(np.median(end_to_end['mesh.save_gif']) / np.median(end_to_end['video.save_gif'])), 2),
            'device_route_stages_s': stages, 'device_route_stages_s_median': {k: float(np.median(v)) for k, v in stages.items()},
            'calls_per_repetition': args.calls, 'entry_point_us': us, 'entry_point_us_median': {k: float(np.median(v)) for k, v in us.items()},
            'palette_rows': n_rows,
            'quantize_gops_per_s': round(pixels * n_rows * 4 / (float(np.median(us['quantize (dither 16)'])) * 1e-6) / 1e9, 1),
            'histogram_gb_per_s': round(pixels * 3 / (float(np.median(us['histogram'])) * 1e-6) / 1e9, 1),
            'files': quality,
            'smooth_clip': {'workload': f'{f} frames of {h} x {w}: the gradients of tests/video_cases.gradient_frames, three grey levels of noise',
                            'end_to_end_s': end_to_end_smooth, 'files': quality_smooth,
                            'speedup': round(end_to_end_smooth['mesh.save_gif'][0] / float(np.median(end_to_end_smooth['video.save_gif'])), 2)},
            'note': 'quantize_gops_per_s counts three multiply-adds and one minimum per pixel and palette row; histogram_gb_per_s the frame bytes read; an entry '
                    'point is all its launches (histogram and box_sums zero their result in a launch of their own)'}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
