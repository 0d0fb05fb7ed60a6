"""A geometry frame of one latent, two ways: the surface cast (``surface.cast`` + ``surface.shade``: the density along 512^2 rays x 128
steps up to the first crossing, 8 bisections) and the path that existed before it, whose API is unchanged (``shape.sigma_grid(512)`` +
``shape.marching_cubes`` + ``mesh.render``).  seg2cat as in tools/bench_texture.py (random weights as in bench.py), the threshold at the
field's median, the cameras of ``views.video_cameras``; the planes are made once, outside every timed window, as an edit session holds them.

    python tools/bench_surface.py [--resolution 512] [--steps 128] [--refine 8] [--views 8] [--reps 5] [--lattice 512] [--out FILE]

Prints ONE JSON line:
  cast_ms / shade_ms              one ``p3d_surface_cast`` launch of one camera (with its ray and decoder-packing launches) / one shaded frame:
                                  device events, median over reps x views after a warm-up; cast_4_views_ms: one launch of four cameras;
  mesh_first_frame_ms             lattice + marching cubes + the first rasterized frame; mesh_next_frame_ms: one more camera of the mesh
                                  (host clock round a synchronised device, median over reps); the two paths alternate inside every repetition;
  depth_agreement                 on a SMOOTH field (planes of 8^2 noise upsampled to 256^2, G's decoder, a 256^3 lattice): the share of the
                                  pixels either path draws at which both draw and the cast's camera-space depth lies within two lattice
                                  steps of the rasterized mesh's.
No number is a pass condition."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return out, a.elapsed_time(b)


def host_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return out, 1e3 * (time.perf_counter() - t0)


def depth_agreement(G, cams, resolution, steps, refine, lattice=256):
    from pix2pix3d_amd import mesh, shape
    from pix2pix3d_amd.training.volumetric_rendering import renderer as rmod
    dev, rk = cams.device, G.rendering_kwargs
    low = torch.randn([1, 96, 8, 8], generator=torch.Generator().manual_seed(5)) * 2
    planes = torch.nn.functional.interpolate(low, size=(256, 256), mode='bicubic', align_corners=False).reshape(1, 3, 32, 256, 256).to(dev)
    bound = rk['box_warp'] * 0.5
    axis = torch.linspace(-bound, bound, lattice)
    u = rmod.fused_sample_lattice(planes, G.decoder, axis, axis, axis, rk)[0]
    thr = float(u.median())
    v, f = shape.marching_cubes(u, thr)
    v = (v.double() / (lattice - 1.0) * (2 * bound) - bound).to(torch.float32)
    cam = cams[:1]
    c2w = cam[:, :16].reshape(1, 4, 4)
    _, fid, zmesh = mesh.render(v, f, c2w, mesh.Pinhole(cam[:, 16:25]), resolution, return_buffers=True)
    ray_o, ray_d = G.ray_sampler(c2w, cam[:, 16:25].reshape(1, 3, 3), resolution)
    hit, t, _, _ = rmod.fused_surface_cast(planes, G.decoder, ray_o, ray_d, rk, rk['ray_start'], rk['ray_end'], steps, refine, thr, rk['box_warp'] / 256, bound,
                                           raster_width=resolution if resolution % 8 == 0 else 0)
    zcast = (t * (ray_d * c2w[0, :3, 2]).sum(-1)).reshape(resolution, resolution)
    drawn_cast, drawn_mesh = hit.reshape(resolution, resolution) != 0, fid[0] >= 0
    close = drawn_cast & drawn_mesh & ((zcast - zmesh[0]).abs() <= 2 * (2 * bound) / (lattice - 1))
    either = int((drawn_cast | drawn_mesh).sum())
    return {'lattice': lattice, 'pixels_either_draws': either, 'pixels_both_draw': int((drawn_cast & drawn_mesh).sum()),
            'share_within_two_steps': round(int(close.sum()) / max(either, 1), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--resolution', type=int, default=512)
    ap.add_argument('--steps', type=int, default=128)
    ap.add_argument('--refine', type=int, default=8)
    ap.add_argument('--views', type=int, default=8)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--lattice', type=int, default=512)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from bench_texture import build
    from pix2pix3d_amd import mesh, shape, surface, views
    assert torch.cuda.is_available(), 'bench_surface.py measures on the GPU'
    dev = torch.device('cuda')
    G = build(dev)
    ws = torch.randn(1, G.backbone.num_ws, 512, generator=torch.Generator().manual_seed(1234)).to(dev)
    res, kw = args.resolution, dict(steps=args.steps, refine=args.refine)
    with torch.no_grad():
        thr = float(shape.sigma_grid(G, ws, 64)[0].median())
        planes = shape._planes(G, ws, noise_mode='const')
        cams = views.video_cameras(G, 'seg2cat', max(args.views, 4)).to(dev)
        c2w, pin = cams[:, :16].reshape(-1, 4, 4), cams[:, 16:25]

        def cast(k, n=1):
            return surface.cast(G, ws, cams[k:k + n], res, threshold=thr, planes=planes, **kw)

        def mesh_first():
            v, f = shape.extract_geometry(G, ws, args.lattice, thr)
            return v, f, mesh.render(v, f, c2w[:1], mesh.Pinhole(pin[:1]), res)

        # warm-up: every shape of the timed windows
        hit = cast(0)
        surface.shade(hit, cams[:1, :16])
        cast(0, 4)
        v, f, _ = mesh_first()
        mesh.render(v, f, c2w[1:2], mesh.Pinhole(pin[1:2]), res)
        t_cast, t_shade, t_cast4, t_first, t_next = [], [], [], [], []
        for _ in range(args.reps):                                      # the two paths alternate inside a repetition
            for k in range(args.views):
                hit, ms = event_ms(lambda: cast(k))
                t_cast.append(ms)
                t_shade.append(event_ms(lambda: surface.shade(hit, cams[k:k + 1, :16]))[1])
            t_cast4.append(event_ms(lambda: cast(0, 4))[1])
            (v, f, _), ms = host_ms(mesh_first)
            t_first.append(ms)
            for k in range(1, min(args.views, 4)):
                t_next.append(host_ms(lambda: mesh.render(v, f, c2w[k:k + 1], mesh.Pinhole(pin[k:k + 1]), res))[1])
        hits = cast(0, args.views)
        agree = depth_agreement(G, cams, res, args.steps, args.refine)
    med = lambda t: round(float(np.median(t)), 3)
    line = {'workload': f'seg2cat, {res}^2 rays x {args.steps} steps, refine {args.refine}, {args.views} cameras, {args.reps} reps; mesh path: lattice {args.lattice}',
            'device': torch.cuda.get_device_name(0), 'threshold': round(thr, 4), 'hit_share': round(float(hits.hit.float().mean()), 4),
            'cast_ms': med(t_cast), 'cast_ms_min_max': [round(min(t_cast), 3), round(max(t_cast), 3)], 'shade_ms': med(t_shade), 'cast_4_views_ms': med(t_cast4),
            'mesh_first_frame_ms': med(t_first), 'mesh_next_frame_ms': med(t_next), 'mesh_vertices': len(v), 'mesh_faces': len(f),
            'depth_agreement': agree}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
