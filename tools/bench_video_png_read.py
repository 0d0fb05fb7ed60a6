"""Reading 120 lossless frames of 512^2 back to device frames, two ways on the same box and the same files:

(a) the loop a user has today: ``PIL.Image.open`` per frame (zlib inflate and libpng-style un-filtering, one core), ``np.asarray``, the frames stacked and
    uploaded in one copy;
(b) ``video.decode_apng`` / ``video.decode_png`` onto the device: chunks parsed on the host, the compressed bytes uploaded in one copy, inflate
    (``p3d_video_png_inflate``, a lane per part), un-filtering (``p3d_video_png_unfilter``, a wave per frame) and the Adler-32 check on the device.

The clips are tools/bench_video_png.py's: the frames of ``views.render_views`` (seg2cat at bench size, random weights, seed 1234) as RGB, the same clip's
``label_index`` as palette indices, and the synthetic continuous-tone RGB clip.  Four device reads a clip: our APNG written with the segment index (a part
a segment), the same frames' APNG without it (one part, so one lane, a frame), Pillow's PNGs of the frames at its default level (foreign streams: one lane
a frame), and a single indexed frame.  The host loop reads the same files (Pillow plays our APNG frame by frame).  End to end: host clock around each
call, which starts with the file on disk (in the page cache) or the list of streams and ends with the frames on the device, after a synchronise; one
warm-up of each, then ``--reps`` repetitions of (b) and ``--pil-reps`` of (a), interleaved; medians.  The kernels: device events around the fill + launch of
``p3d_video_png_inflate`` and the launch of ``p3d_video_png_unfilter`` (``_lib.kernel_timer``), medians.  Every device read is checked against the frames.

    python tools/bench_video_png_read.py [--frames 120] [--reps 7] [--pil-reps 2] [--out profiles/video_png_read_bench.json]

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

KERNELS = ('video_png_inflate', 'video_png_unfilter')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=120)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--pil-reps', type=int, default=2)
    ap.add_argument('--synthetic-only', action='store_true', help='leave the generator out: the synthetic clip alone')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from PIL import Image
    from pix2pix3d_amd import _lib, mesh, video
    assert torch.cuda.is_available(), 'bench_video_png_read.py measures the device kernels: it needs the GPU'
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

    def pil_file(path):
        """Every frame of the file as PIL shows it, stacked and uploaded."""
        with Image.open(path) as im:
            frames = []
            for i in range(getattr(im, 'n_frames', 1)):
                im.seek(i)
                frames.append(np.asarray(im).copy())
        return torch.from_numpy(np.stack(frames)).to(dev)

    def pil_streams(streams):
        return torch.from_numpy(np.stack([np.asarray(Image.open(io.BytesIO(s))) for s in streams])).to(dev)

    def measure(ours, theirs, frames):
        _, a = seconds(ours)
        _, b = seconds(theirs)
        t_dev, t_pil = [], []
        for name in KERNELS:
            _lib.kernel_events[name] = []
        for rep in range(max(args.reps, args.pil_reps)):
            if rep < args.pil_reps:
                t_pil.append(seconds(theirs)[0])
            if rep < args.reps:
                t_dev.append(seconds(ours)[0])
        kernel_us = {name: [round(e0.elapsed_time(e1) * 1e3, 1) for e0, e1 in _lib.kernel_events.pop(name)] for name in KERNELS}
        return {'device_s': [round(t, 4) for t in t_dev], 'host_loop_s': [round(t, 4) for t in t_pil], 'device_s_median': float(np.median(t_dev)),
                'host_loop_s_median': float(np.median(t_pil)), 'speedup_median': round(float(np.median(t_pil) / np.median(t_dev)), 2), 'kernel_us': kernel_us,
                'kernel_us_median': {k: float(np.median(v)) for k, v in kernel_us.items()}, 'device_exact': bool(torch.equal(a, frames)),
                'host_loop_exact': bool(torch.equal(b, frames))}

    clips = {'synthetic RGB': (gradient_clip(args.frames, 512, 512), None, None)}
    if not args.synthetic_only:
        from bench_views import build
        from pix2pix3d_amd import views
        G = build(dev)
        ws = torch.randn(1, G.backbone.num_ws, 512, generator=torch.Generator().manual_seed(1234)).to(dev)
        cams = views.video_cameras(G, 'seg2cat', args.frames).to(dev)
        rendered = views.render_views(G, ws, cams, views_per_step=4, neural_rendering_resolution=128, noise_mode='const')
        clips['rendered RGB'] = (rendered['image'], None, None)
        clips['rendered label indices'] = (rendered['label_index'], 'P', mesh.default_palette(256))
    tmp = tempfile.mkdtemp()
    results = {}
    for name, (frames, mode, palette) in clips.items():
        indexed, plain = os.path.join(tmp, 'indexed.png'), os.path.join(tmp, 'plain.png')
        video.save_apng(indexed, frames, mode=mode, palette=palette, index=True)
        video.save_apng(plain, frames, mode=mode, palette=palette)
        foreign = []
        for a in frames.cpu().numpy():
            im = Image.fromarray(a)
            if mode == 'P':
                im.putpalette(palette.numpy().tobytes())                              # (an 'L' image becomes 'P' with it)
            out = io.BytesIO()
            im.save(out, 'PNG')
            foreign.append(out.getvalue())
        one = video.encode_png(frames[:1], mode=mode, palette=palette, index=True)
        info = video.png_parse(one[0])
        results[name] = {
            'our APNG, indexed': dict(measure(lambda: video.decode_apng(indexed, device=dev)[0], lambda: pil_file(indexed), frames),
                                      file_bytes=os.path.getsize(indexed), parts_a_frame=len(info.index[0][1]) + 1),
            'our APNG, no index': dict(measure(lambda: video.decode_apng(plain, device=dev)[0], lambda: pil_file(plain), frames),
                                       file_bytes=os.path.getsize(plain), parts_a_frame=1),
            "Pillow's PNGs": dict(measure(lambda: video.decode_png(foreign, device=dev), lambda: pil_streams(foreign), frames),
                                  file_bytes=sum(map(len, foreign)), parts_a_frame=1),
            'one indexed frame': dict(measure(lambda: video.decode_png(one, device=dev), lambda: pil_streams(one), frames[:1]),
                                      file_bytes=len(one[0]), parts_a_frame=len(info.index[0][1]) + 1)}

    for name, rows in results.items():
        print(f'{name}, {args.frames} frames of 512 x 512')
        for what, r in rows.items():
            print(f'  {what:22s} {r["file_bytes"]:10d} bytes, {r["parts_a_frame"]:3d} parts a frame: host loop {r["host_loop_s_median"]:8.4f} s, device {r["device_s_median"]:8.4f} s '
                  f'({r["speedup_median"]}x); inflate {r["kernel_us_median"]["video_png_inflate"]:9.1f} us, un-filter {r["kernel_us_median"]["video_png_unfilter"]:9.1f} us; '
                  f'exact {r["device_exact"]} / {r["host_loop_exact"]}')
    line = {'workload': f'{args.frames} frames of 512 x 512 (tools/bench_video_png.py\'s clips), written losslessly four ways and read back: the file or the streams in, '
                        'device frames out', 'device': torch.cuda.get_device_name(0), 'host_cpus_used_by_the_host_loop': 1, 'segment_bytes': video.PNG_SEGMENT_BYTES,
            'inflate_lanes_a_work_group': video.PNG_INFLATE_LANES, 'results': results,
            'note': 'host_loop = PIL.Image.open per frame (seek for an APNG), np.asarray, np.stack, one upload; device route = decode_apng / decode_png with '
                    'verify=True; kernel_us are device events around the fill + launch of png_inflate and the launch of png_unfilter inside the timed calls'}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
