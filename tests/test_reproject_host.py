"""pix2pix3d_amd.reproject on CPU tensors: the torch formulations (the definition the device bytes are held to in test_reproject_gpu.py) against the
brute-force restatement of reproject_cases.py, the rules on planted cases (drops, ties, statuses), an analytic sphere seen from two cameras, the formulas of
``metrics_from_consistency`` by hand, and the argument errors — those of the Python surface and those of the built library, which come before any device call."""
import ctypes
import math

import numpy as np
import pytest
import torch

from reproject_cases import EMPTY, PLANTED, brute_differences, brute_resolve, brute_splat, cameras_at, planted_points, sphere_scene, view_in_canvas

ANGLES = [(0.0, 0.0), (0.1, -0.05), (-0.2, 0.1)]
SOURCE, TARGET = (24, 20), (17, 29)


@pytest.fixture(scope='module')
def planted():
    """(points [3, 24, 20, 3], cameras [3, 25], valid [3, 24, 20]): shared, never modified."""
    valid = (torch.rand(3, *SOURCE, generator=torch.Generator().manual_seed(1)) < 0.7).to(torch.uint8) * 5
    return planted_points(3, *SOURCE), cameras_at(ANGLES), valid


@pytest.fixture(scope='module')
def spheres():
    return sphere_scene([(0.0, 0.0), (0.1, -0.05), (0.35, 0.0)], 64)


# ---- 1. the formulations against brute force -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('radius', [0, 1, 2])
@pytest.mark.parametrize('with_valid', [False, True])
@pytest.mark.parametrize('broadcast', [False, True])
def test_splat_equals_brute_force(planted, radius, with_valid, broadcast):
    from pix2pix3d_amd import reproject
    pts, cams, valid = planted
    pts, valid = (pts[:1], valid[:1]) if broadcast else (pts, valid)
    valid = valid if with_valid else None
    got = reproject.splat(pts, cams, size=TARGET, radius=radius, valid=valid)
    want = brute_splat(pts, cams, TARGET, radius, valid)
    covered = int((want != EMPTY).sum())
    print('radius', radius, 'valid', with_valid, 'broadcast', broadcast, 'covered', covered, 'of', want.size, 'differing', int((got.numpy() != want).sum()))
    assert got.dtype == torch.int64 and tuple(got.shape) == (3, *TARGET) and np.array_equal(got.numpy(), want)
    assert 0 < covered and (radius == 2 or covered < want.size)
    if broadcast and valid is None:
        assert np.array_equal(reproject.splat(pts[0], cams, size=TARGET, radius=radius).numpy(), want)         # [h, w, 3]


def test_planted_drops_never_land(planted):
    from pix2pix3d_amd import reproject
    pts, cams, _ = planted
    zbuf = reproject.splat(pts, cams, size=TARGET, radius=2)
    landed = set((zbuf[zbuf != EMPTY] & 0xffffffff).tolist())
    assert landed and not landed & set(PLANTED)
    only = torch.stack([torch.tensor(p) for p in PLANTED.values()]).view(1, 1, len(PLANTED), 3).expand(3, -1, -1, -1).contiguous()
    assert bool((reproject.splat(only, cams, size=TARGET, radius=2) == EMPTY).all())
    near = torch.tensor([0.0, 0.0, 2.7 - 1.0 / 65536]).view(1, 1, 1, 3)                                            # zc = 2^-16 .. : the smallest keys
    assert int(reproject.splat(near, cams[:1], size=(1, 1)).item()) >> 32 in (0, 1)


def test_ties_go_to_the_smaller_index_and_the_nearer_point_wins(planted):
    from pix2pix3d_amd import reproject
    cams = planted[1][:1]
    depth_of = {2: 1.5, 5: 1.0, 9: 1.0, 11: 2.0}                                                                   # index -> zc along the central ray
    pts = torch.full([1, 1, 12, 3], float('nan'))
    for i, d in depth_of.items():
        pts[0, 0, i] = torch.tensor([0.0, 0.0, 2.7 - d])
    zbuf = reproject.splat(pts, cams, size=TARGET)
    centre = int(zbuf[0, TARGET[0] // 2, TARGET[1] // 2])
    assert centre & 0xffffffff == 5 and abs((centre >> 32) - 65536) <= 1 and int((zbuf != EMPTY).sum()) == 1
    pts[0, 0, 11, 2] = 2.7 - 0.5                                                                                   # the last index, but nearer
    assert int(reproject.splat(pts, cams, size=TARGET)[0, TARGET[0] // 2, TARGET[1] // 2]) & 0xffffffff == 11
    again = reproject.splat(pts, cams, size=TARGET, out=zbuf)                                                      # into a buffer that holds keys already
    assert again is zbuf and int(zbuf[0, TARGET[0] // 2, TARGET[1] // 2]) & 0xffffffff == 11


@pytest.mark.parametrize('channels', [1, 3, 4])
def test_resolve_equals_brute_force(planted, channels):
    from pix2pix3d_amd import reproject
    pts, cams, valid = planted
    zbuf = reproject.splat(pts, cams, size=TARGET, radius=1, valid=valid)
    source = torch.randint(0, 256, [3, *SOURCE, channels], generator=torch.Generator().manual_seed(2), dtype=torch.uint8)
    fill = [9, 8, 7, 6][:channels]
    target = planted_points(3, *TARGET, seed=5)
    for src, tgt in ((source, None), (source, target), (source[:1], target), (view_in_canvas(source, 3), target)):
        counts = torch.zeros(5, dtype=torch.int64)
        got = reproject.resolve(zbuf, src, fill, tgt, cams if tgt is not None else None, 3000 if tgt is not None else None, counts=counts, return_index=True)
        want = brute_resolve(zbuf, src, fill, tgt, cams, 3000)
        for g, w, name in zip(got, want, ('warped', 'status', 'index')):
            assert np.array_equal(g.numpy(), w), name
        assert got[0].dtype == torch.uint8 and got[1].dtype == torch.uint8 and got[2].dtype == torch.int32
        assert torch.equal(counts, torch.bincount(got[1].reshape(-1).long(), minlength=5))
        assert tgt is None or len(set(got[1].unique().tolist())) >= 4
    canvas = view_in_canvas(torch.full([3, *TARGET, channels], 77, dtype=torch.uint8), 1)
    got, _ = reproject.resolve(zbuf, source, fill, out=canvas)                                                   # the caller's pitched view
    assert got is canvas and torch.equal(canvas, reproject.resolve(zbuf, source, fill)[0])
    for bad in (canvas[:2], canvas.int(), canvas.permute(0, 2, 1, 3), source):
        with pytest.raises(ValueError):
            reproject.resolve(zbuf, source if bad is not source else torch.zeros([3, *TARGET, channels], dtype=torch.uint8), fill, out=bad)
    with pytest.raises(ValueError, match='out of place'):
        reproject.resolve(reproject.splat(pts, cams), source, fill, out=source)                                   # a target of the source's size, written onto it
    if channels == 1:
        plain = reproject.resolve(zbuf, source[..., 0], 9)
        assert tuple(plain[0].shape) == (3, *TARGET) and torch.equal(plain[0], reproject.resolve(zbuf, source, 9)[0][..., 0])


def test_difference_histogram_equals_brute_force():
    from pix2pix3d_amd import reproject
    g = torch.Generator().manual_seed(3)
    a, b = torch.randint(0, 256, [2, 13, 11, 3], generator=g, dtype=torch.uint8), torch.randint(0, 256, [2, 13, 11, 3], generator=g, dtype=torch.uint8)
    where = torch.randint(0, 3, [2, 13, 11], generator=g, dtype=torch.uint8)
    for w, match in ((None, 1), (where, 1), (where, 2), (where, 200)):
        got = reproject.difference_histogram(a, b, w, match)
        assert np.array_equal(got.numpy(), brute_differences(a, b, w, match))
    assert int(reproject.difference_histogram(a, b).sum()) == a.numel() and int(reproject.difference_histogram(a, b, where, 200).sum()) == 0
    out = reproject.difference_histogram(a[..., 0].contiguous(), b[..., 0].contiguous())
    assert reproject.difference_histogram(a[0, :, :, 0].contiguous(), b[0, :, :, 0].contiguous(), out=out) is out and int(out.sum()) == 3 * 13 * 11
    assert torch.equal(reproject.difference_histogram(a, a), torch.tensor([a.numel()] + [0] * 255))


# ---- 2. the sphere -----------------------------------------------------------------------------------------------------------------------
def test_a_view_warped_into_its_own_camera_is_itself(spheres):
    """Every pixel covered, consistent at tolerance 0, labels and image reproduced exactly: float32 ``points`` moves no pixel across a ``floor`` boundary."""
    from pix2pix3d_amd import reproject
    s = spheres
    zbuf = reproject.splat(s['points'], s['cameras'])
    own = torch.arange(64 * 64).view(1, 64, 64).expand(3, -1, -1)
    assert torch.equal(zbuf & 0xffffffff, own)
    labels, status = reproject.resolve(zbuf, s['labels'], 255, s['points'], s['cameras'], 0)
    images, _ = reproject.resolve(zbuf, s['images'], 0)
    assert bool((status == reproject.CONSISTENT).all()) and torch.equal(labels, s['labels']) and torch.equal(images, s['images'])
    total = reproject.consistency_counts(s['labels'], s['images'], s['depth'], s['cameras'], [(0, 0), (1, 1), (2, 2)], 8, 0)
    r = total.result()
    assert r['coverage'] == 1.0 and r['consistent'] == 1.0 and r['in_front'] == 0.0 and r['labels']['accuracy'] == 1.0 and r['mad'] == 0.0 and r['psnr'] == float('inf')
    assert torch.equal(r['labels']['matrix'], torch.diag(r['labels']['matrix'].diagonal())) and r['pairs'] == 3


@pytest.mark.parametrize('pair', [(0, 1), (0, 2)])
def test_a_turned_pair_agrees_where_it_is_covered(spheres, pair):
    """Yaw +0.1 rad, pitch -0.05 (and yaw 0.35): sanity conditions that keep the test from being vacuous, not tolerances on a kernel."""
    from pix2pix3d_amd import reproject
    s = spheres
    r = reproject.consistency_counts(s['labels'], s['images'], s['depth'], s['cameras'], [pair], 8, round(0.02 * 65536)).result()
    print(pair, {k: r[k] for k in ('coverage', 'consistent', 'behind', 'in_front', 'mad', 'psnr')}, 'accuracy', r['labels']['accuracy'])
    assert r['coverage'] > 0.5 and int(r['status_counts'][reproject.IN_FRONT]) == 0 and r['labels']['accuracy'] > 0.99
    assert r['pixels'] == 64 * 64 and r['covered'] == int(r['status_counts'][1:].sum()) and r['labels']['pixels'] == int(r['status_counts'][1])


def test_warp_is_points_splat_resolve(spheres):
    from pix2pix3d_amd import reproject
    s = spheres
    warped, status = reproject.warp(s['images'][0], s['depth'][0], s['cameras'][0], s['cameras'][1:], radius=1, fill=3)
    zbuf = reproject.splat(s['points'][:1], s['cameras'][1:], radius=1)
    want, want_status = reproject.resolve(zbuf, s['images'][:1], 3)
    assert tuple(warped.shape) == (2, 64, 64, 3) and torch.equal(warped, want) and torch.equal(status, want_status)
    assert int((status == 0).sum()) < int((reproject.resolve(reproject.splat(s['points'][:1], s['cameras'][1:]), s['images'][:1])[1] == 0).sum())
    flat, _ = reproject.warp(s['labels'][0], s['depth'][0], s['cameras'][0], s['cameras'][1:])
    assert tuple(flat.shape) == (2, 64, 64)


def test_status_rule_with_planted_target_points(spheres):
    """A farther target point: the source is in front (3); a nearer one: behind (2); an invalid one: 4; the counts are the bincount."""
    from pix2pix3d_amd import reproject
    s = spheres
    cams, pts = s['cameras'][:1], s['points'][:1]
    zbuf = reproject.splat(pts, cams)
    eye = cams[0, [3, 7, 11]]
    along = pts - eye
    for scale, want in ((1.05, reproject.IN_FRONT), (0.95, reproject.BEHIND), (float('nan'), reproject.NO_TARGET), (1.0, reproject.CONSISTENT)):
        counts = torch.zeros(5, dtype=torch.int64)
        _, status = reproject.resolve(zbuf, s['labels'][:1], 0, (eye + along * scale).contiguous(), cams, 100, counts=counts)
        assert bool((status == want).all()) and counts.tolist() == [64 * 64 if k == want else 0 for k in range(5)]
    mixed = pts.clone()
    mixed[0, :16] = eye + along[0, :16] * 1.05
    mixed[0, 16:32] = eye + along[0, 16:32] * 0.95
    mixed[0, 32:40] = float('inf')
    zbuf[0, 60:] = EMPTY
    counts = torch.zeros(5, dtype=torch.int64)
    _, status = reproject.resolve(zbuf, s['labels'][:1], 0, mixed, cams, 100, counts=counts)
    assert counts.tolist() == [4 * 64, 20 * 64, 16 * 64, 16 * 64, 8 * 64] and torch.equal(counts, torch.bincount(status.reshape(-1).long(), minlength=5))


# ---- 3. the formulas ---------------------------------------------------------------------------------------------------------------------
def test_metrics_by_hand():
    from pix2pix3d_amd import reproject
    status = torch.tensor([10, 60, 20, 6, 4])
    confusion = torch.tensor([30, 5, 0, 25, 0])                                     # two labels: truth 0 -> 30 right, 5 wrong; truth 1 -> 25 right
    differences = torch.zeros(256, dtype=torch.int64)
    differences[0], differences[2], differences[10] = 170, 8, 2
    r = reproject.metrics_from_consistency(status, confusion, differences)
    assert r['pixels'] == 100 and r['covered'] == 90 and r['coverage'] == 0.9
    assert r['consistent'] == 60 / 90 and r['behind'] == 20 / 90 and r['in_front'] == 6 / 90 and r['no_target'] == 4 / 90
    assert r['labels']['accuracy'] == 55 / 60 and r['labels']['miou'] == (30 / 35 + 25 / 30) / 2
    assert r['mad'] == (2 * 8 + 10 * 2) / 180 and r['mse'] == (4 * 8 + 100 * 2) / 180 and r['psnr'] == 10 * math.log10(255.0 * 255.0 / (232 / 180))
    empty = reproject.metrics_from_consistency(torch.zeros(5, dtype=torch.int64), torch.zeros(5, dtype=torch.int64), torch.zeros(256, dtype=torch.int64))
    for key in ('coverage', 'consistent', 'behind', 'in_front', 'no_target', 'mad', 'mse', 'psnr'):
        assert math.isnan(empty[key]), key
    assert math.isnan(empty['labels']['accuracy']) and empty['pixels'] == 0
    holes = reproject.metrics_from_consistency(torch.tensor([7, 0, 0, 0, 0]), None, torch.zeros(256, dtype=torch.int64))
    assert holes['coverage'] == 0.0 and math.isnan(holes['in_front']) and holes['labels'] is None
    same = reproject.metrics_from_consistency(status, None, torch.tensor([5] + [0] * 255))
    assert same['mad'] == 0.0 and same['psnr'] == float('inf')
    with pytest.raises(ValueError):
        reproject.metrics_from_consistency(status[:4], None, differences)


def test_default_tolerance_is_one_coarse_sample_spacing():
    from pix2pix3d_amd import reproject

    class G:
        rendering_kwargs = dict(ray_start=2.25, ray_end=3.3, depth_resolution=48)
    assert reproject.default_tolerance(G) == round(65536 * 1.05 / 48) == 1434


def test_turned_camera_is_rigid_about_the_pivot():
    from pix2pix3d_amd import reproject
    cam = cameras_at([(0.0, 0.0)])
    pivot = [0.0, 0.0, 0.2]
    turned = reproject.turned_camera(cam, pivot, yaw=0.3, pitch=-0.1, roll=0.05)
    m0, m1 = cam[0, :16].view(4, 4).double(), turned[0, :16].view(4, 4).double()
    p = torch.tensor(pivot, dtype=torch.float64)
    assert torch.allclose(m1[:3, :3].T @ m1[:3, :3], torch.eye(3, dtype=torch.float64), atol=1e-6) and torch.equal(turned[0, 16:], cam[0, 16:])
    assert torch.allclose(m1[:3, :3].T @ (p - m1[:3, 3]), m0[:3, :3].T @ (p - m0[:3, 3]), atol=1e-6)         # the pivot stays where it was in the camera's frame
    assert torch.equal(reproject.turned_camera(cam, pivot), cam)


# ---- 4. argument errors ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_python_surface(planted):
    from pix2pix3d_amd import reproject
    pts, cams, valid = planted
    zbuf = reproject.splat(pts, cams, size=TARGET)
    source = torch.zeros([3, *SOURCE, 3], dtype=torch.uint8)
    frames = torch.zeros([3, *TARGET, 3], dtype=torch.uint8)
    bad = [lambda: reproject.splat(pts.double(), cams), lambda: reproject.splat(pts[..., :2], cams), lambda: reproject.splat(pts, cams[:, :24]),
           lambda: reproject.splat(pts, cams[:2]), lambda: reproject.splat(pts, cams.double()), lambda: reproject.splat(pts, cams, radius=3),
           lambda: reproject.splat(pts, cams, radius=-1), lambda: reproject.splat(pts, cams, radius=1.5), lambda: reproject.splat(pts, cams, size=(0, 5)),
           lambda: reproject.splat(pts, cams, size=(5, 4097)), lambda: reproject.splat(pts, cams, valid=valid[:, :, :19]),
           lambda: reproject.splat(pts, cams, valid=valid.float()), lambda: reproject.splat(pts, cams, valid=valid[:2]),
           lambda: reproject.splat(pts.permute(0, 2, 1, 3), cams),                                                       # points of a frame not contiguous
           lambda: reproject.splat(torch.as_strided(pts, pts.shape, (30, 60, 3, 1)), cams),                             # frames that overlap
           lambda: reproject.splat(pts, cams, valid=torch.as_strided(valid, valid.shape, (100, 20, 1))),                # frames that overlap
           lambda: reproject.splat(pts, cams, valid=torch.as_strided(valid, valid.shape, (480, 19, 1))),                # rows that overlap
           lambda: reproject.splat(pts, cams, size=TARGET, out=torch.zeros([3, *TARGET], dtype=torch.int32)),
           lambda: reproject.splat(pts, cams, size=TARGET, out=torch.zeros([3, TARGET[1], TARGET[0]], dtype=torch.int64)),
           lambda: reproject.splat(pts, cams, size=TARGET, out=torch.zeros([3, TARGET[0], 2 * TARGET[1]], dtype=torch.int64)[:, :, ::2]),
           lambda: reproject.resolve(zbuf.int(), source), lambda: reproject.resolve(zbuf, source.float()), lambda: reproject.resolve(zbuf, source[:2]),
           lambda: reproject.resolve(zbuf, torch.zeros([3, *SOURCE, 5], dtype=torch.uint8)), lambda: reproject.resolve(zbuf, source, fill=256),
           lambda: reproject.resolve(zbuf, source, fill=[1, 2]), lambda: reproject.resolve(zbuf, source.permute(0, 2, 1, 3)),
           lambda: reproject.resolve(zbuf, source, target_points=pts), lambda: reproject.resolve(zbuf, source, cameras=cams),
           lambda: reproject.resolve(zbuf, source, target_points=pts, cameras=cams, tolerance=5),                          # target points of the source's size
           lambda: reproject.resolve(zbuf, source, target_points=planted_points(3, *TARGET), cameras=cams, tolerance=-1),
           lambda: reproject.resolve(zbuf, source, target_points=planted_points(3, *TARGET), cameras=cams, tolerance=1 << 31),
           lambda: reproject.resolve(zbuf, source, counts=torch.zeros(4, dtype=torch.int64)),
           lambda: reproject.difference_histogram(frames, frames[:2]), lambda: reproject.difference_histogram(frames, frames.float()),
           lambda: reproject.difference_histogram(frames, frames, where=torch.zeros([3, *TARGET, 1], dtype=torch.uint8)),
           lambda: reproject.difference_histogram(frames, frames, where=torch.zeros([3, TARGET[1], TARGET[0]], dtype=torch.uint8)),
           lambda: reproject.difference_histogram(frames, frames, match=256), lambda: reproject.difference_histogram(frames, frames, out=torch.zeros(255, dtype=torch.int64)),
           lambda: reproject.difference_histogram(torch.zeros([3, 4, 4, 5], dtype=torch.uint8), torch.zeros([3, 4, 4, 5], dtype=torch.uint8)),
           lambda: reproject.consistency_counts(None, frames, torch.zeros(3, 17, 17), cams, [(0, 3)], None, 5),
           lambda: reproject.consistency_counts(None, frames, torch.zeros(3, 17, 17), cams, [(0, 1)], None, 5, out=reproject.Consistency(4, 'cpu')),
           lambda: reproject.points(torch.zeros(3, 17, 29), cams), lambda: reproject.points(torch.zeros(2, 16, 16), cams)]
    for k, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
            print('call', k, 'raised nothing')
    assert bool((reproject.splat(pts[:0], cams[:0], size=TARGET).numel() == 0))


def test_argument_errors_of_the_library_come_before_any_launch():
    from pix2pix3d_amd import _lib, regions
    lib = regions.regions_lib()
    n0 = regions.launch_count()
    p = ctypes.c_void_p(4096)                                                       # never read: every call below fails its argument check (or has no frames)
    fill = (ctypes.c_uint8 * 4)(1, 2, 3, 4)
    splat = lambda points=p, pitch=1440, valid=None, v_row=0, v_frame=0, cams=p, frames=2, h=24, w=20, radius=0, zbuf=p, H=17, W=29: \
        lib.p3d_view_splat(points, pitch, valid, v_row, v_frame, cams, frames, h, w, radius, zbuf, H, W, None)
    resolve = lambda zbuf=p, src=p, s_row=60, s_frame=1440, h=24, w=20, c=3, fill=fill, dst=ctypes.c_void_p(1 << 20), d_row=87, d_frame=1479, index=None, \
        status=p, target=None, cams=None, tol=0, counts=None, frames=2, H=17, W=29: \
        lib.p3d_view_resolve(zbuf, src, s_row, s_frame, h, w, c, fill, dst, d_row, d_frame, index, status, target, cams, tol, counts, frames, H, W, None)
    diff = lambda a=p, a_row=87, a_frame=1479, b=p, b_row=87, b_frame=1479, where=None, w_row=0, w_frame=0, match=1, c=3, frames=2, H=17, W=29, hist=p: \
        lib.p3d_view_difference_histogram(a, a_row, a_frame, b, b_row, b_frame, where, w_row, w_frame, match, c, frames, H, W, hist, None)
    bad = [splat(points=None), splat(cams=None), splat(zbuf=None), splat(radius=3), splat(radius=-1), splat(frames=-1), splat(frames=65537), splat(h=0), splat(W=4097),
           splat(pitch=1439), splat(valid=p, v_row=19, v_frame=480), splat(valid=p, v_row=20, v_frame=479), splat(zbuf=ctypes.c_void_p(4100)),
           splat(points=ctypes.c_void_p(4097)),
           resolve(zbuf=None), resolve(src=None), resolve(dst=None), resolve(status=None), resolve(fill=None), resolve(c=5), resolve(c=0), resolve(s_row=59),
           resolve(s_frame=1439), resolve(d_row=86), resolve(d_frame=1478), resolve(target=p), resolve(target=p, cams=p, tol=-1), resolve(target=p, cams=p, tol=1 << 31),
           resolve(dst=ctypes.c_void_p(4096 + 100)), resolve(H=0), resolve(frames=65537), resolve(index=ctypes.c_void_p(4098)),
           diff(a=None), diff(b=None), diff(hist=None), diff(c=5), diff(match=256), diff(match=-1), diff(a_row=86), diff(b_frame=1478), diff(where=p, w_row=28, w_frame=493),
           diff(where=p, w_row=29, w_frame=492), diff(W=0), diff(frames=-1), diff(hist=ctypes.c_void_p(4100))]
    assert all(code == _lib.P3D_ERR_ARGUMENT for code in bad), [k for k, code in enumerate(bad) if code != _lib.P3D_ERR_ARGUMENT]
    with pytest.raises(RuntimeError, match='libp3d_regions error -2: view_splat: radius'):
        regions._check(splat(radius=3), 'view_splat')
    assert splat(frames=0, points=None, cams=None, zbuf=None) == resolve(frames=0, zbuf=None, src=None, dst=None, status=None) == diff(frames=0, a=None, b=None) == _lib.P3D_OK
    assert regions.launch_count() == n0


def test_the_three_entry_points_live_in_the_regions_library_and_nowhere_else():
    """Declared by p3d_regions.h after the six it had, exported by libp3d_regions.so, bound by ``regions.regions_lib()`` itself (no import of reproject needed),
    absent from the product ABI; the status codes and EMPTY are the header's constants and reproject's names follow them."""
    import json
    import pathlib
    import subprocess
    import sys
    from pix2pix3d_amd import _lib, build, regions, reproject
    names = ['p3d_view_splat', 'p3d_view_resolve', 'p3d_view_difference_histogram']
    assert list(regions.HEADER.functions)[-3:] == names and len(regions.HEADER.functions) == 9
    assert not set(names) & set(_lib.HEADER.functions)
    assert [len(regions.HEADER.functions[n][1]) for n in names] == [14, 21, 16]
    paths = build.side_paths('regions')
    assert [h.name for h in pathlib.Path(paths.src_dir).glob('*.h')] == ['p3d_regions.h'] and (pathlib.Path(paths.src_dir) / 'view_reproject.hip').is_file()
    assert '#include "p3d_' not in pathlib.Path(paths.header).read_text()
    side, product = ctypes.CDLL(paths.lib), ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert hasattr(side, name) and not hasattr(product, name), name
    child = ('import json; from pix2pix3d_amd import regions; raw = regions.regions_lib()._handle; '
             'print(json.dumps([n for n in regions.HEADER.functions if getattr(raw, n).argtypes is None])); import sys; assert "pix2pix3d_amd.reproject" not in sys.modules')
    r = subprocess.run([sys.executable, '-c', child], capture_output=True, text=True, cwd=pathlib.Path(_lib.LIB_PATH).parent.parent)
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout.strip().splitlines()[-1]) == []
    assert (reproject.EMPTY, reproject.HOLE, reproject.CONSISTENT, reproject.BEHIND, reproject.IN_FRONT, reproject.NO_TARGET) == ((1 << 63) - 1, 0, 1, 2, 3, 4)
    assert (reproject.GUARD, reproject.MAX_RADIUS, reproject.MAX_CHANNELS, reproject.MAX_FRAMES, reproject.MAX_TOLERANCE) == (4, 2, 4, 65536, (1 << 31) - 1)
    assert 'p3d_view' not in pathlib.Path(_lib.LIB_PATH).with_name('..').resolve().joinpath('include', 'p3d_hip.h').read_text()
