"""A texture atlas for one latent's extracted mesh, per stage, beside the per-vertex path it extends: the lattice-512 seg2cat mesh of
tools/bench_texture.py (threshold at the field's median, random weights as in bench.py), decimated with ``mesh.simplify`` so that its
faces fit the atlas (a 2048^2 atlas holds at most 524 288 faces, at cells of 4 texels; the lattice-512 mesh has millions), 24 views at
512^2, everything on the device — orient (``atlas.orient_faces``), texel geometry (``p3d_mesh_atlas_texels``), the bake of the K texels
(project + rasterize of the mesh, project of the texels, ``p3d_mesh_bake_accumulate``, finish), assemble (``p3d_mesh_atlas_assemble``)
and the script's 120-frame 512^2 turntable with the texture (``atlas.render_textured``; its last stage, ``p3d_mesh_shade_textured``,
also alone) — and, on the same mesh, frames and cameras, the parent path: ``texture.bake_colors`` and ``mesh.render`` (``p3d_mesh_shade``).

    python tools/bench_atlas.py [--lattice 512] [--cell 0.0078125] [--size 2048] [--views 24] [--frames 120] [--reps 3] [--out FILE]

Prints ONE JSON line: the sizes and the median wall time of every stage in ms over ``--reps`` repetitions after a warm-up (host timer
around a synchronised device).  No time is a pass condition."""
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lattice', type=int, default=512)
    ap.add_argument('--cell', type=float, default=1 / 128, help='mesh.simplify cell in world units, enlarged by quarters until the faces fit (0: no decimation)')
    ap.add_argument('--size', type=int, default=2048)
    ap.add_argument('--views', type=int, default=24)
    ap.add_argument('--frames', type=int, default=120)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from bench_texture import build
    from pix2pix3d_amd import atlas, mesh, shape, texture, views
    dev = torch.device('cuda')
    G = build(dev)
    ws = torch.randn(1, G.backbone.num_ws, 512, generator=torch.Generator().manual_seed(1234)).to(dev)

    def timed(fn, reps=args.reps):
        out, times = None, []
        for k in range(reps + 1):                                      # the first call warms up
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            if k:
                times.append(1e3 * (time.perf_counter() - t0))
        return out, round(float(np.median(times)), 3)

    thr = float(shape.sigma_grid(G, ws, 64)[0].median())
    v0, f0 = shape.extract_geometry(G, ws, args.lattice, thr)
    stage = {}
    cell = args.cell
    while True:                                                         # decimate until the faces fit the atlas
        (v, f), stage['simplify'] = timed(lambda: mesh.simplify(v0, f0, cell)) if cell > 0 else ((v0, f0), 0.0)
        try:
            lay = atlas.layout(len(f), args.size)
            break
        except ValueError:
            if cell <= 0:
                raise
            cell *= 1.25
    f, stage['orient_faces'] = timed(lambda: atlas.orient_faces(v, f))
    cams = texture.bake_cameras(G, 'seg2cat', args.views).to(dev)
    c2w, cam = cams[:, :16].reshape(-1, 4, 4), mesh.Pinhole(cams[:, 16:25])
    frames = views.render_views(G, ws, cams, jitter='frozen', noise_mode='const', neural_rendering_resolution=128)['image']
    res = frames.shape[1]
    normals = texture.vertex_normals(v, f)
    (points, tnormals, face), stage['texel_points'] = timed(lambda: atlas.texel_points(v, f, normals, lay))
    (proj, fid, dep), stage['project_rasterize_mesh'] = timed(lambda: (lambda p: (p,) + mesh.rasterize(p, f, res))(mesh.project(v, c2w, cam, res)))
    tproj, stage['project_texels'] = timed(lambda: mesh.project(points, c2w, cam, res))
    acc, seen = texture.bake_buffers(lay.n_texels, dev)

    def accumulate():
        acc.zero_(); seen.zero_()
        texture.bake_accumulate(acc, seen, tproj, fid, dep, frames, points, tnormals, c2w)
    _, stage['accumulate_texels'] = timed(accumulate)
    colors, stage['finish_texels'] = timed(lambda: texture.bake_finish(acc))
    _, stage['assemble'] = timed(lambda: atlas.assemble(colors, face, lay))
    seen_share = round(float((seen[face >= 0] > 0).float().mean()), 4)
    del proj, tproj, fid, dep, acc, seen, colors
    (tex, _), stage['bake_texture_whole'] = timed(lambda: atlas.bake_texture(v, f, frames, c2w, cam, lay, normals=normals))
    poses, tcam = mesh.script_turntable(G, args.frames)
    _, stage['render_textured'] = timed(lambda: atlas.render_textured(v, f, poses, tcam, 512, tex, lay))
    proj = mesh.project(v, poses, tcam, 512)
    fid, _ = mesh.rasterize(proj, f, 512)
    _, stage['shade_textured_alone'] = timed(lambda: atlas.shade_textured(fid, proj, v, f, poses, tex, lay))
    parent = {}
    vcol, parent['bake_colors_whole'] = timed(lambda: texture.bake_colors(v, f, frames, c2w, cam, normals=normals))
    _, parent['render'] = timed(lambda: mesh.render(v, f, poses, tcam, 512, colors=vcol))
    _, parent['shade_alone'] = timed(lambda: mesh.shade(fid, proj, v, f, poses, vcol))

    line = {'workload': f'seg2cat lattice {args.lattice} simplified at cell {cell:g}, atlas {args.size}^2, {args.views} views at {res}^2, '
                        f'{args.frames} turntable frames at 512^2', 'device': torch.cuda.get_device_name(0),
            'lattice_faces': len(f0), 'vertices': len(v), 'faces': len(f), 'atlas_cell': lay.cell, 'texels': lay.n_texels,
            'seen_share_of_texels': seen_share, 'stage_ms': stage, 'per_vertex_path_ms': parent}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(text + '\n')


if __name__ == '__main__':
    main()
