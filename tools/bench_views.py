"""A 120-frame video of one latent, two ways on the same box: (a) the loop of the reference's applications/generate_video.py restated — ``G.synthesis(ws, pose)``
per frame, ``.cpu()``, the numpy finishing with a ``color_mask``-style palette loop — and (b) ``views.render_views`` (backbone once, shared-plane chunks, frames
finished on the device) at ``views_per_step`` 1, 4 and 8, frames left on the device and again with one final copy to the host.  seg2cat at bench size: 128^2
rays x 64+64 samples, 512^2 frames, six label channels, random weights as in bench.py.  Three interleaved repetitions of each after a warm-up.

    python tools/bench_views.py [--frames 120] [--reps 3] [--out profiles/views_bench.json]

Prints ONE JSON line: frames/s of every variant per repetition, the per-stage device times of (b) per chunk (backbone once, ray-marcher launch, heads, finishing
launch; HIP events), the ray-marcher's time PER VIEW in the shared-plane launch against the equal-batch launch at B = 4 (interleaved, same draws), and the two
conditions: (b) at views_per_step = 4 faster than (a) in every repetition pair, and the finishing launch of a B = 4 chunk within the time its own bytes need
at a tenth of the 8 TB/s HBM peak (4 x 11.2 MB / 0.8 TB/s = 56 us)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build(device):
    import importlib.util
    from pix2pix3d_amd import configs, dnnlib
    spec = importlib.util.spec_from_file_location('p3d_weights', os.path.join(ROOT, 'tests', 'golden', 'weights.py'))
    w = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(w)
    torch.manual_seed(0)
    G = dnnlib.util.construct_class_by_name(**configs.generator_kwargs('seg2cat', depth=(64, 64))).eval().requires_grad_(False)
    w.seed_module(G, seed=1)
    return G.to(device)


def script_loop(G, ws, cams, palette):
    """(a): generate_video.py:57-67 per frame, with the palette loop of training/utils.py:5-15."""
    frames, labels = [], []
    for k in range(len(cams)):
        with torch.no_grad():
            out = G.synthesis(ws, cams[k:k + 1], noise_mode='const', neural_rendering_resolution=128)
        image = out['image'][0].permute(1, 2, 0).cpu().numpy()
        frames.append(((np.clip(image, -1, 1) + 1) * 127.5).astype(np.uint8))
        index = torch.argmax(out['semantic'], dim=1).cpu().numpy()[0]
        colour = np.zeros(index.shape + (3,))
        for c in range(len(palette)):
            colour[index == c] = palette[c]
        labels.append(colour.astype(np.uint8))
    return frames, labels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=120)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from pix2pix3d_amd import views, mesh, _lib
    from pix2pix3d_amd.training.volumetric_rendering import renderer as rmod
    dev = torch.device('cuda')
    G = build(dev)
    ws = torch.randn(1, G.backbone.num_ws, 512, generator=torch.Generator().manual_seed(1234)).to(dev)
    cams = views.video_cameras(G, 'seg2cat', args.frames).to(dev)
    palette = mesh.default_palette(6).numpy()
    F = args.frames

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return F / (time.perf_counter() - t0)

    def native(step, to_host):
        def run():
            out = views.render_views(G, ws, cams, views_per_step=step, neural_rendering_resolution=128, noise_mode='const')
            if to_host:
                return {k: v.cpu() for k, v in out.items()}
            return out
        return run

    variants = {'script_loop': lambda: script_loop(G, ws, cams, palette)}
    for step in (1, 4, 8):
        variants[f'render_views_{step}'] = native(step, False)
        variants[f'render_views_{step}_to_host'] = native(step, True)
    script_loop(G, ws, cams[:8], palette)                              # warm-up: every kernel, every allocation size
    for step in (1, 4, 8):
        views.render_views(G, ws, cams[:2 * step], views_per_step=step, neural_rendering_resolution=128, noise_mode='const')
    fps = {k: [] for k in variants}
    for _ in range(args.reps):                                         # interleaved
        for k, fn in variants.items():
            fps[k].append(round(timed(fn), 2))

    # per-stage device times of (b) at views_per_step = 4, HIP events on the stream everything is launched on
    stage = {'backbone': [], 'render': [], 'heads': []}

    def hook(mod, key):
        def pre(m, a):
            e = torch.cuda.Event(enable_timing=True); e.record(); m._bv_e0 = e

        def post(m, a, o):
            e = torch.cuda.Event(enable_timing=True); e.record(); stage[key].append((m._bv_e0, e))
        return [mod.register_forward_pre_hook(pre), mod.register_forward_hook(post)]
    handles = hook(G.backbone.synthesis, 'backbone') + hook(G.renderer, 'render') + hook(G.superresolution, 'heads') + hook(G.superresolution_semantic, 'heads')
    _lib.kernel_events['render_forward'], _lib.kernel_events['frame_finish'] = [], []
    views.render_views(G, ws, cams, views_per_step=4, neural_rendering_resolution=128, noise_mode='const')
    torch.cuda.synchronize()
    for h in handles:
        h.remove()
    kern, fin = _lib.kernel_events.pop('render_forward'), _lib.kernel_events.pop('frame_finish')
    chunks = len(kern)
    ms = lambda pairs: [a.elapsed_time(b) for a, b in pairs]
    fin_us = sorted(1e3 * t for t in ms(fin))
    stage_ms = {'backbone_once': round(sum(ms(stage['backbone'])), 3), 'renderer_per_chunk': round(sum(ms(stage['render'])) / chunks, 3),
                'ray_marcher_launch_per_chunk': round(sum(ms(kern)) / chunks, 3), 'heads_per_chunk': round(sum(ms(stage['heads'])) / chunks, 3),
                'finish_launch_us_median': round(fin_us[len(fin_us) // 2], 1), 'finish_launch_us_max': round(fin_us[-1], 1), 'chunks': chunks}

    # the ray-marcher alone: shared planes [1] x 4 cameras against the equal-batch launch [4] x 4 cameras, interleaved, same rays and draws
    with torch.no_grad():
        planes = G.backbone_planes(ws, noise_mode='const')
        planes = planes.view(1, 3, 32, planes.shape[-2], planes.shape[-1])
        rep = planes.expand(4, -1, -1, -1, -1).contiguous()
        c = cams[::max(1, F // 4)][:4]
        o, d = G.ray_sampler(c[:, :16].view(-1, 4, 4), c[:, 16:25].view(-1, 3, 3), 128)
        u_c, u_f = torch.rand(4, 128 * 128, 64, 1, device=dev), torch.rand(4 * 128 * 128, 64, device=dev)
        per_view = {'shared': [], 'equal_batch': []}
        for it in range(12):
            for key, p in (('shared', planes), ('equal_batch', rep)):
                _lib.kernel_events['render_forward'] = []
                rmod.fused_render(p, G.decoder, o, d, G.rendering_kwargs, u_c, u_f)
                torch.cuda.synchronize()
                (a, b), = _lib.kernel_events.pop('render_forward')
                if it >= 2:
                    per_view[key].append(a.elapsed_time(b) / 4)
    ray = {k: {'ms_per_view_median': round(float(np.median(v)), 4), 'ms_per_view_min': round(min(v), 4)} for k, v in per_view.items()}

    cap_us = 4 * 11.2e6 / 0.8e12 * 1e6
    line = {'workload': f'seg2cat, {F} frames of one latent, 128^2 rays x 64+64 samples -> 512^2, 6 label channels', 'device': torch.cuda.get_device_name(0),
            'frames_per_s': fps, 'stage_ms_views_per_step_4': stage_ms, 'ray_marcher_b4': ray,
            'conditions': {'render_views_4_faster_than_script_loop_in_every_pair': all(b > a for a, b in zip(fps['script_loop'], fps['render_views_4'])),
                           'finish_launch_cap_us': round(cap_us, 1), 'finish_launch_within_cap': stage_ms['finish_launch_us_median'] <= cap_us}}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
