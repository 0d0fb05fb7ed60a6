"""Two events of an interactive edit, two ways on the same box: "40 new strokes -> frame on the host" and "camera moved -> frame on the host".

(a) the sequence of the reference's applications/demo/qt_demo_seg2cat.py restated (:371-399, 429-463): every stroke ever drawn is repainted on the host and the
    mask copied to the device, the whole ``G.mapping`` runs through the one-hot route, then the whole ``G.synthesis`` — for a camera move too —, ``.cpu()``, numpy
    clip / scale, ``argmax``, ``.cpu()`` and the palette loop.  No cv2 exists here: the host painter is the CPU formulation of ``edit.paint_strokes`` (the integer
    capsule rule, each stroke inside its bounding box), not ``cv2.line``; the palette loop is ``color_mask``'s (one boolean mask per label, training/utils.py:5-15),
    as in tools/bench_views.py, not the demo's 512^2 ``setPixel`` calls.  Both stand-ins are cheaper than what they stand for.
(b) ``edit.EditSession``: one ``p3d_paint_strokes`` launch, the label entry + Encoder, the backbone, the ray-marcher and heads over the kept planes, one finishing
    launch, one copy of the uint8 frame.  A camera move runs only the last three.

seg2cat at bench size (512^2 mask, six labels, 128^2 rays x 64+64 samples, random weights as in bench.py).  The log holds 160 strokes before every edit event; an event
replaces its last 40 by 40 new ones.  ``--reps`` interleaved repetitions of ``--events`` events each after a warm-up; host clock around work that ends in the copy to the host.

    python tools/bench_edit.py [--reps 3] [--events 8] [--out profiles/edit_bench.json]

Prints ONE JSON line: ms per event of both variants per repetition, and the per-stage device times of (b) (HIP events): paint, label entry, Encoder, backbone,
ray-marcher, heads, finish."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def brush_strokes(k, seed, n_labels=6, size=512):
    """k brush segments: runs of short moves with one thickness and label, as a mouse drag records them."""
    r = np.random.RandomState(seed)
    out, pos = [], r.randint(60, size - 60, 2)
    for i in range(k):
        if i % 10 == 0:
            pos, t, label = r.randint(60, size - 60, 2), int(r.randint(8, 50)), int(r.randint(0, n_labels))
        nxt = np.clip(pos + r.randint(-18, 19, 2), 0, size - 1)
        out.append((int(pos[0]), int(pos[1]), int(nxt[0]), int(nxt[1]), t, label))
        pos = nxt
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--events', type=int, default=8)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from bench_views import build
    from pix2pix3d_amd import edit, mesh, configs, _lib
    dev = torch.device('cuda')
    G = build(dev)
    rk = G.rendering_kwargs
    r = np.random.RandomState(0)
    base = torch.from_numpy(np.repeat(np.repeat(r.randint(0, 6, [64, 64]).astype(np.uint8), 8, axis=0), 8, axis=1).copy())
    pose = torch.from_numpy(configs.orbit_camera(9, radius=rk['avg_camera_radius'], pivot=rk['avg_camera_pivot']))
    palette = mesh.default_palette(6).numpy()
    earlier = brush_strokes(160, seed=1)
    z = torch.from_numpy(np.random.RandomState(0).randn(1, G.z_dim).astype('float32')).to(dev)
    fwd = edit.forward_label(G).to(dev)
    intrinsics = pose[16:25].reshape(3, 3)
    yaws = [20 + 7 * k for k in range(64)]

    def label_for(yaw):
        return torch.cat([edit.camera_from_euler(*edit.slider_angles(yaw=yaw, pitch=50)).reshape(1, 16), intrinsics.reshape(1, 9)], dim=1).to(dev)

    # ---- (a) the demo's sequence -----------------------------------------------------------------------------------------
    demo = {'ws': None}

    def demo_generate(c):
        with torch.no_grad():
            out = G.synthesis(demo['ws'], c, noise_mode='const', neural_rendering_resolution=128)
        img = ((out['image'].permute(0, 2, 3, 1).squeeze(0).cpu().numpy().clip(-1, 1) * 0.5 + 0.5) * 255).astype(np.uint8).copy()
        index = torch.argmax(out['semantic'].detach(), dim=1).cpu().numpy()[0]
        colour = np.zeros(index.shape + (3,))
        for k in range(len(palette)):
            colour[index == k] = palette[k]
        return img, colour.astype(np.uint8), index.astype(np.uint8)

    def demo_edit(strokes, c):
        mask = edit.paint_strokes(base, earlier[:120] + strokes)              # every stroke ever drawn, on the host
        with torch.no_grad():
            demo['ws'] = G.mapping(z, fwd, {'mask': mask[None, None].to(dev), 'pose': pose[None].to(dev)})
        return demo_generate(c)

    # ---- (b) the session -------------------------------------------------------------------------------------------------
    s = edit.EditSession(G, cfg='seg2cat', seed=0, hold_texture=False)
    s.load(base, pose)
    s.paint(earlier[:120])
    s.paint(earlier[120:])

    def session_edit(strokes, yaw):
        s.undo()
        s.paint(strokes)
        s.set_camera(yaw=yaw, pitch=50)
        return s.frame()

    def session_camera(yaw):
        s.set_camera(yaw=yaw, pitch=50)
        return s.frame()

    def timed(fn, items):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for it in items:
            fn(it)
        torch.cuda.synchronize()
        return round((time.perf_counter() - t0) * 1e3 / len(items), 3)

    n = args.events
    new = [brush_strokes(40, seed=100 + k) for k in range((args.reps + 1) * n)]
    variants = {
        'edit_demo': lambda k: demo_edit(new[k], label_for(yaws[k % 64])),
        'edit_session': lambda k: session_edit(new[k], yaws[k % 64]),
        'camera_demo': lambda k: demo_generate(label_for(yaws[(k + 3) % 64])),
        'camera_session': lambda k: session_camera(yaws[(k + 3) % 64]),
    }
    for key, fn in variants.items():                                          # warm-up: every kernel, every allocation size
        timed(fn, range(2))
    ms = {k: [] for k in variants}
    for rep in range(args.reps):                                              # interleaved
        for key, fn in variants.items():
            ms[key].append(timed(fn, range((rep + 1) * n, (rep + 2) * n)))

    # ---- per-stage device times of (b): one edit event, then one camera event ---------------------------------------------------
    stage = {k: [] for k in ('encoder', 'backbone', 'renderer', 'heads')}

    def hook(mod, key):
        def pre(m, a):
            e = torch.cuda.Event(enable_timing=True); e.record(); m._be_e0 = e

        def post(m, a, o):
            e = torch.cuda.Event(enable_timing=True); e.record(); stage[key].append((m._be_e0, e))
        return [mod.register_forward_pre_hook(pre), mod.register_forward_hook(post)]
    handles = hook(G.backbone.mapping.embed_mask, 'encoder') + hook(G.backbone.synthesis, 'backbone') + hook(G.renderer, 'renderer') \
        + hook(G.superresolution, 'heads') + hook(G.superresolution_semantic, 'heads')
    kernels = ('paint_strokes', 'label_features', 'render_forward', 'frame_finish')
    span = lambda pairs: round(sum(a.elapsed_time(b) for a, b in pairs), 3)
    stage_ms = {}
    for event, run in (('edit', lambda: session_edit(new[0], 33)), ('camera', lambda: session_camera(47))):
        for k in stage:
            stage[k] = []
        for k in kernels:
            _lib.kernel_events[k] = []
        n0 = _lib.launch_count()
        run()
        torch.cuda.synchronize()
        logs = {k: _lib.kernel_events.pop(k) for k in kernels}
        stage_ms[event] = {'paint_launch': span(logs['paint_strokes']), 'label_entry_launch': span(logs['label_features']), 'encoder': span(stage['encoder']),
                           'backbone': span(stage['backbone']), 'renderer': span(stage['renderer']), 'ray_marcher_launch': span(logs['render_forward']),
                           'heads': span(stage['heads']), 'finish_launch': span(logs['frame_finish']), 'library_launches': _lib.launch_count() - n0}
    for h in handles:
        h.remove()

    med = {k: float(np.median(v)) for k, v in ms.items()}
    line = {'workload': 'seg2cat edit events: 512^2 mask, 6 labels, 160 strokes in the log of which 40 are new, 128^2 rays x 64+64 samples -> 512^2 frame on the host',
            'device': torch.cuda.get_device_name(0), 'events_per_repetition': n, 'ms_per_event': ms, 'ms_per_event_median': med,
            'demo_over_session': {'edit': round(med['edit_demo'] / med['edit_session'], 3), 'camera': round(med['camera_demo'] / med['camera_session'], 3)},
            'session_stage_ms': stage_ms,
            'host_painter': 'CPU formulation of edit.paint_strokes (no cv2 on this box)', 'palette_loop': 'one boolean mask per label (color_mask), not 512^2 setPixel calls'}
    text = json.dumps(line)
    print(text)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
