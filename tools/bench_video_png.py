"""Writing a 120-frame 512^2 clip losslessly, two ways on the same box and the same device frames:

(a) the host loop the feature replaces, written out here: ``frames[i].cpu()`` and ``PIL.Image.save`` per frame, at PIL's default level — the way
    ``views.generate_sample`` writes a PNG; the copy is part of the time.  Its bytes also at ``compress_level=1``;
(b) ``video.save_apng`` and ``video.save_png_sequence``: row filter, symbol counts and deflate bytes on the device (libp3d_video.so), one Huffman code a frame
    made on the host in between, only the compressed bytes copied.

Three clips: the frames of ``views.render_views`` (seg2cat at bench size, random weights as in bench.py, seed 1234) as RGB; the same clip's ``label_index`` as
palette indices (mode 'P' against PIL's 'P'); and a synthetic continuous-tone RGB clip — tests/video_cases.gradient_frames' formula made on the device — since
a random-weight generator paints smoother frames than a trained one.  End to end: host clock around each call, which starts with device frames and ends with
the file(s) written, after a synchronise; one warm-up of each, then ``--reps`` repetitions of (b) and ``--pil-reps`` of (a), interleaved; medians.  The kernels:
device events around the one launch of each stage in every repetition of ``save_apng`` (``_lib.kernel_timer``), medians.  ``video.PNG_SEGMENT_BYTES`` is swept
over 8192, 16384 and 32768 for time and size; everything else runs at the module's default.

    python tools/bench_video_png.py [--frames 120] [--reps 7] [--pil-reps 2] [--out profiles/video_png_bench.json]

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
sys.path.insert(0, os.path.join(ROOT, 'tools'))

SEGMENT_BYTES = (8192, 16384, 32768)
KERNELS = ('video_png_filter', 'video_png_count', 'video_png_emit')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=120)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--pil-reps', type=int, default=2)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from PIL import Image
    from bench_views import build
    from pix2pix3d_amd import _lib, mesh, video, views
    assert torch.cuda.is_available(), 'bench_video_png.py measures the device kernels: it needs the GPU'
    dev = torch.device('cuda')
    G = build(dev)
    ws = torch.randn(1, G.backbone.num_ws, 512, generator=torch.Generator().manual_seed(1234)).to(dev)
    cams = views.video_cameras(G, 'seg2cat', args.frames).to(dev)
    rendered = views.render_views(G, ws, cams, views_per_step=4, neural_rendering_resolution=128, noise_mode='const')
    palette = mesh.default_palette(256)

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

    tmp = tempfile.mkdtemp()

    def host_loop(frames, pal, **save):
        """The parent's way: one device -> host copy and one PIL save a frame.  Returns the files' bytes in all."""
        total = 0
        for i in range(frames.shape[0]):
            im = Image.fromarray(frames[i].cpu().numpy(), 'P' if pal is not None else None)
            if pal is not None:
                im.putpalette(pal.numpy().tobytes())
            path = os.path.join(tmp, f'pil_{i:04d}.png')
            im.save(path, **save)
            total += os.path.getsize(path)
        return total

    clips = {'rendered RGB': (rendered['image'], None, None), 'rendered label indices': (rendered['label_index'], 'P', palette),
             'synthetic RGB': (gradient_clip(args.frames, 512, 512), None, None)}
    results = {}
    default_segment = video.PNG_SEGMENT_BYTES
    for name, (frames, mode, pal) in clips.items():
        apng = lambda: video.save_apng(os.path.join(tmp, 'clip.png'), frames, mode=mode, palette=pal)
        sequence = lambda: video.save_png_sequence(os.path.join(tmp, 'dev_{:04d}.png'), frames, mode=mode, palette=pal)
        seconds(apng), seconds(sequence)                                           # warm-up: code objects, allocation sizes, pinned memory
        pil_bytes = seconds(lambda: host_loop(frames, pal))[1]
        pil_bytes_level1 = host_loop(frames, pal, compress_level=1)
        t_apng, t_seq, t_pil = [], [], []
        for k in KERNELS:
            _lib.kernel_events[k] = []
        for rep in range(max(args.reps, args.pil_reps)):
            if rep < args.pil_reps:
                t_pil.append(seconds(lambda: host_loop(frames, pal))[0])
            if rep < args.reps:
                t_apng.append(seconds(apng)[0])
        kernel_us = {k: [round(e0.elapsed_time(e1) * 1e3, 1) for e0, e1 in _lib.kernel_events.pop(k)] for k in KERNELS}
        for rep in range(args.reps):
            t_seq.append(seconds(sequence)[0])
        stream_bytes = sum(map(len, apng()))
        sweep = {}
        for segment in SEGMENT_BYTES:
            video.PNG_SEGMENT_BYTES = segment
            seconds(apng)
            times = [seconds(apng)[0] for _ in range(args.reps)]
            sweep[str(segment)] = {'save_apng_s': [round(t, 4) for t in times], 'save_apng_s_median': float(np.median(times)), 'stream_bytes': sum(map(len, apng())),
                                   'segments_a_frame': -(-frames.shape[1] // video.png_segment_rows(frames.shape[2], frames.shape[3] if frames.ndim == 4 else 1))}
        video.PNG_SEGMENT_BYTES = default_segment
        results[name] = {
            'frames': int(frames.shape[0]), 'raw_bytes': int(frames.numel()), 'segment_bytes': default_segment,
            'save_apng_s': [round(t, 4) for t in t_apng], 'save_png_sequence_s': [round(t, 4) for t in t_seq], 'host_loop_s': [round(t, 4) for t in t_pil],
            'save_apng_s_median': float(np.median(t_apng)), 'save_png_sequence_s_median': float(np.median(t_seq)), 'host_loop_s_median': float(np.median(t_pil)),
            'speedup_median': round(float(np.median(t_pil) / np.median(t_apng)), 2),
            'kernel_us': kernel_us, 'kernel_us_median': {k: float(np.median(v)) for k, v in kernel_us.items()},
            'bytes': {'device_streams': stream_bytes, 'apng_file': os.path.getsize(os.path.join(tmp, 'clip.png')), 'pil_default': pil_bytes,
                      'pil_compress_level_1': pil_bytes_level1},
            'device_over_pil_default': round(stream_bytes / pil_bytes, 4), 'segment_sweep': sweep}

    for name, r in results.items():
        print(f'{name}, {r["frames"]} frames of 512 x 512, {r["raw_bytes"]} raw bytes')
        print(f'  {"host loop (copy + PIL save), s, median":50s}{r["host_loop_s_median"]:10.4f}   {r["bytes"]["pil_default"]:10d} bytes '
              f'({r["bytes"]["pil_compress_level_1"]} at compress_level=1)')
        print(f'  {"video.save_apng, s, median":50s}{r["save_apng_s_median"]:10.4f}   {r["bytes"]["device_streams"]:10d} bytes   ({r["speedup_median"]}x, '
              f'{r["device_over_pil_default"]} of PIL\'s bytes)')
        print(f'  {"video.save_png_sequence, s, median":50s}{r["save_png_sequence_s_median"]:10.4f}')
        for k, v in r['kernel_us_median'].items():
            print(f'  {k:50s}{v:10.1f} us')
        for segment, s in r['segment_sweep'].items():
            print(f'  {"PNG_SEGMENT_BYTES = " + segment:50s}{s["save_apng_s_median"]:10.4f}   {s["stream_bytes"]:10d} bytes, {s["segments_a_frame"]} segments a frame')
    line = {'workload': f'{args.frames} frames of 512 x 512: views.render_views (seg2cat at bench size, random weights, seed 1234) as RGB and as label indices, and a '
                        'synthetic continuous-tone RGB clip; device frames in, files written out',
            'device': torch.cuda.get_device_name(0), 'host_cpus_used_by_the_host_loop': 1, 'results': results,
            'note': 'host_loop = frames[i].cpu() and PIL.Image.save per frame at the default level; kernel_us are device events around single launches inside the '
                    'timed save_apng calls (the event pair is on only during this measurement); device_over_pil_default compares zlib streams with whole files'}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
