"""Time mesh rendering on the GPU (pix2pix3d_amd/mesh.py, csrc/mesh_raster.hip) and print ONE JSON line.

The seeded config-size seg2cat generator (configs.generator_kwargs, tests/golden/weights.py: no checkpoint is needed), its mesh at the
median of the 512^3 density field (shape.extract_geometry), the script's turntable (orthographic xmag 0.3, radius 1, 512^2).  Device
events after a warm-up, medians of the repetitions:
  project_ms / raster_ms / shade_ms   one frame through each stage (raster: count, scan, host copy of the total, bin, raster)
  turntable_120_ms                    mesh.render of all 120 frames end to end (projections in groups of at most 1 GiB)
  write_ply_ms                        mesh.write_ply of that mesh with vertex colours (host clock, to a temporary file)
  cpu_*                               the CPU path on a small case for scale: a 64^3 sphere, 8 frames at 128^2 (host clock)
Usage: python tools/time_mesh_render.py [--reps 5]
"""
import argparse
import importlib.util
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

from pix2pix3d_amd import configs, dnnlib, mesh, shape  # noqa: E402


def _generator(name):
    spec = importlib.util.spec_from_file_location('p3d_weights', os.path.join(ROOT, 'tests', 'golden', 'weights.py'))
    weights = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(weights)
    torch.manual_seed(0)
    G = dnnlib.util.construct_class_by_name(**configs.generator_kwargs(name)).eval().requires_grad_(False)
    weights.seed_module(G, seed=1)
    return G.cuda()


def _ms(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def _median(fn, reps):
    fn()
    torch.cuda.synchronize()
    return statistics.median(_ms(fn)[0] for _ in range(reps))


def _host_median(fn, reps):
    fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=5)
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'time_mesh_render.py measures on the GPU'
    t_start = time.time()
    out = {'tool': 'time_mesh_render', 'device': torch.cuda.get_device_name(0), 'reps': args.reps}
    G = _generator('seg2cat')
    ws = torch.randn([1, G.backbone.num_ws, 512], generator=torch.Generator().manual_seed(0)).cuda()
    with torch.no_grad():
        thr = float(shape.sigma_grid(G, ws, 512)[0].median())
        v, f = shape.extract_geometry(G, ws, 512, thr)
        colors = mesh.vertex_labels(G, ws, v)[1]
    out.update(threshold=thr, vertices=int(v.shape[0]), faces=int(f.shape[0]))
    poses = mesh.turntable_poses(G.rendering_kwargs['avg_camera_pivot'], 1.0, 120)
    cam = mesh.Orthographic(0.3, 0.3)
    f32 = f.to(torch.int32)
    one = poses[:1]
    proj = mesh.project(v, one, cam, 512)
    fid, _ = mesh.rasterize(proj, f32, 512)
    out['project_ms'] = _median(lambda: mesh.project(v, one, cam, 512), args.reps)
    out['raster_ms'] = _median(lambda: mesh.rasterize(proj, f32, 512), args.reps)
    out['shade_ms'] = _median(lambda: mesh.shade(fid, proj, v, f32, one, colors), args.reps)
    out['silhouette_px_frame0'] = int((fid >= 0).sum())
    out['turntable_120_ms'] = _median(lambda: mesh.render(v, f, poses, cam, 512, colors=colors), args.reps)
    frames = mesh.render(v, f, poses, cam, 512, colors=colors)
    out['turntable_empty_frames'] = int(((frames != 255).any(-1).sum(dim=(1, 2)) == 0).sum())
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, 'mesh.ply')
        out['write_ply_ms'] = _host_median(lambda: mesh.write_ply(path, v, f, colors), max(1, args.reps // 2))
        out['ply_bytes'] = os.path.getsize(path)
    del frames, proj, fid
    # the CPU path, for scale
    g = torch.stack(torch.meshgrid(*[torch.arange(64, dtype=torch.float32)] * 3, indexing='ij'), -1)
    sv, sf = shape.marching_cubes(25.0 - (g - 31.6).norm(dim=-1), 0.0)
    sv = sv / 63 - 0.5
    sp = mesh.turntable_poses([0, 0, 0], 1.0, 8)
    out['cpu_faces'] = int(sf.shape[0])
    out['cpu_render_8x128_ms'] = _host_median(lambda: mesh.render(sv, sf, sp, mesh.Orthographic(0.6, 0.6), 128), 3)
    svd, sfd = sv.cuda(), sf.cuda()
    out['gpu_render_8x128_ms'] = _median(lambda: mesh.render(svd, sfd, sp, mesh.Orthographic(0.6, 0.6), 128), args.reps)
    out['wall_s'] = round(time.time() - t_start, 1)
    print(json.dumps(out))


if __name__ == '__main__':
    main()
