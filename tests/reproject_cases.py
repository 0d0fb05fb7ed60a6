"""Shared by test_reproject_host.py / test_reproject_gpu.py (and tools/bench_reproject.py): the first-principles restatement of pix2pix3d_amd.reproject in
numpy — the projection with fp64 scalars in the header's order, the splat as Python loops over points and footprint pixels, the resolve as a loop over target
pixels — and the scenes: an analytic sphere seen by cameras that look at it, and random points with planted drops."""
import numpy as np
import torch

EMPTY = np.iinfo(np.int64).max
FOCAL, CAMERA_RADIUS, SPHERE_RADIUS = 4.2647, 2.7, 0.5        # video_cameras' focal and camera radius; the sphere sits at the origin and fills every view


def cameras_at(angles, radius=CAMERA_RADIUS, focal=FOCAL):
    """float32 [F, 25]: cameras looking at the origin from ``radius``, one per (yaw, pitch) in radians."""
    from pix2pix3d_amd import edit, views
    poses = torch.stack([edit.camera_from_euler(0.0, yaw, pitch, radius) for yaw, pitch in angles])
    return views.camera_labels(poses, torch.tensor([[focal, 0, 0.5], [0, focal, 0.5], [0, 0, 1]], dtype=torch.float32))


def sphere_depth(cameras, size):
    """float32 [F, size, size]: the exact hit distance (computed in float64) of every pixel's ray with the sphere; every ray hits."""
    from pix2pix3d_amd.training.volumetric_rendering.ray_sampler import RaySampler
    o, d = RaySampler()(cameras[:, :16].view(-1, 4, 4), cameras[:, 16:25].view(-1, 3, 3), size)
    o, d = o.double(), d.double()
    b, c = (o * d).sum(-1), (o * o).sum(-1) - SPHERE_RADIUS ** 2
    t = -b - torch.sqrt(b * b - c)
    assert bool(torch.isfinite(t).all())
    return t.float().view(-1, size, size)


def octant_labels(points):
    """uint8 [...]: the octant of a world point, 0 .. 7."""
    return ((points[..., 0] > 0).to(torch.uint8) + 2 * (points[..., 1] > 0).to(torch.uint8) + 4 * (points[..., 2] > 0).to(torch.uint8))


def shaded_image(points):
    """uint8 [..., 3]: a colour that is a smooth function of the world point."""
    return ((points * 0.9 + 0.5).clamp(0, 1) * 255).to(torch.uint8)


def sphere_scene(angles, size):
    """dict of CPU tensors: cameras [F, 25], depth [F, s, s], points [F, s, s, 3], labels [F, s, s], images [F, s, s, 3]."""
    from pix2pix3d_amd import reproject
    cams = cameras_at(angles)
    depth = sphere_depth(cams, size)
    pts = reproject.points(depth, cams)
    return {'cameras': cams, 'depth': depth, 'points': pts, 'labels': octant_labels(pts), 'images': shaded_image(pts)}


PLANTED = {0: (float('nan'), 0.0, 0.0), 1: (0.0, float('inf'), 0.0), 2: (0.0, 0.0, float('-inf')), 3: (0.0, 0.0, 5.0),       # (3: behind the cameras at z = +2.7)
           4: (0.0, 0.0, -40000.0), 5: (100.0, 0.0, 0.0), 6: (0.0, -60.0, 0.1)}                                             # farther than 2^15; far outside the image


def planted_points(frames, h, w, seed=0):
    """float32 [frames, h, w, 3]: random points in the cube about the origin (the cameras of ``cameras_at`` see its middle; its rim falls outside the image and
    partly outside the guard band), with the ``PLANTED`` drops at the first indices of every frame."""
    g = torch.Generator().manual_seed(seed)
    pts = (torch.rand(frames, h * w, 3, generator=g) - 0.5) * torch.tensor([1.3, 1.3, 1.0])
    for i, p in PLANTED.items():
        pts[:, i] = torch.tensor(p)
    return pts.view(frames, h, w, 3)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def project_point(p, cam, size):
    """(sx, sy, zs, ok) of one point: fp64 scalars, one rounding per operator, the header's order."""
    h, w = size
    with np.errstate(all='ignore'):
        m = [np.float64(v) for v in cam]
        x, y, z = (np.float64(v) for v in p)
        qx, qy, qz = x - m[3], y - m[7], z - m[11]
        xc = m[0] * qx; xc = xc + m[4] * qy; xc = xc + m[8] * qz
        yc = m[1] * qx; yc = yc + m[5] * qy; yc = yc + m[9] * qz
        zc = m[2] * qx; zc = zc + m[6] * qy; zc = zc + m[10] * qz
        a = m[16] * xc; a = a + m[17] * yc
        u = a / zc + m[18]
        v = (m[20] * yc) / zc + m[21]
        zs = zc * np.float64(65536.0)
        ok = bool(np.isfinite(x) and np.isfinite(y) and np.isfinite(z) and zc > 0 and zs < 2147483648.0)
        return np.floor(u * np.float64(w)), np.floor(v * np.float64(h)), zs, ok


def brute_splat(points, cameras, size, radius=0, valid=None, zbuf=None):
    """int64 [F, H, W] by loops over frames, points and footprint pixels.  points [F or 1, h, w, 3], valid [F or 1, h, w] or None."""
    pts, cams = np.asarray(points, np.float32), np.asarray(cameras, np.float32)
    f, (h, w) = cams.shape[0], size
    n = pts.shape[1] * pts.shape[2]
    pts = pts.reshape(pts.shape[0], n, 3)
    val = None if valid is None else np.asarray(valid).reshape(np.asarray(valid).shape[0], n)
    out = np.full([f, h, w], EMPTY, np.int64) if zbuf is None else zbuf
    for k in range(f):
        for i in range(n):
            if val is not None and val[k % val.shape[0], i] == 0:
                continue
            sx, sy, zs, ok = project_point(pts[k % pts.shape[0], i], cams[k], size)
            if not (ok and -4 <= sx < w + 4 and -4 <= sy < h + 4):
                continue
            key = (int(np.floor(zs)) << 32) + i
            for ty in range(int(sy) - radius, int(sy) + radius + 1):
                for tx in range(int(sx) - radius, int(sx) + radius + 1):
                    if 0 <= tx < w and 0 <= ty < h and key < out[k, ty, tx]:
                        out[k, ty, tx] = key
    return out


def brute_resolve(zbuf, source, fill, target=None, cameras=None, tolerance=0):
    """(warped [F, H, W, C], status [F, H, W], index [F, H, W]) by a loop over the target pixels.  source [F or 1, h, w, C]."""
    z, src = np.asarray(zbuf), np.asarray(source)
    f, h, w = z.shape
    s, sh, sw, c = src.shape
    flat = src.reshape(s, sh * sw, c)
    warped, status, index = np.zeros([f, h, w, c], np.uint8), np.zeros([f, h, w], np.uint8), np.full([f, h, w], -1, np.int32)
    for k in range(f):
        for ty in range(h):
            for tx in range(w):
                key = int(z[k, ty, tx])
                i, zk = key & 0xffffffff, key >> 32
                if i >= sh * sw:
                    warped[k, ty, tx] = fill
                    continue
                warped[k, ty, tx], index[k, ty, tx], st = flat[k % s, i], i, 1
                if target is not None:
                    _, _, zs, ok = project_point(np.asarray(target, np.float32)[k, ty, tx], np.asarray(cameras, np.float32)[k], (h, w))
                    zt = int(np.floor(zs)) if ok else 0
                    st = 4 if not ok else (1 if abs(zk - zt) <= tolerance else (2 if zk > zt else 3))
                status[k, ty, tx] = st
    return warped, status, index


def brute_differences(a, b, where=None, match=1):
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    d = np.abs(a - b)
    if where is not None:
        d = d[np.asarray(where) == match]
    hist = np.zeros(256, np.int64)
    np.add.at(hist, d.ravel(), 1)
    return hist


def view_in_canvas(frames, shift, pad=7):
    """``frames`` uint8 [N, h, w(, C)] as a view with padded rows and frames and a pointer ``shift`` bytes off, inside a canvas of 77s (CPU; move it with
    ``views_cases.to_device_same_layout``)."""
    t = frames if frames.ndim == 4 else frames[..., None]
    n, h, w, c = t.shape
    row, frame = (w + 2) * c + pad, (h + 2) * ((w + 2) * c + pad) + 5
    store = torch.full([n * frame + 8], 77, dtype=torch.uint8)
    view = torch.as_strided(store, [n, h, w, c], [frame, row, c, 1], shift + row + c)
    view.copy_(t)
    return view if frames.ndim == 4 else view[..., 0]
