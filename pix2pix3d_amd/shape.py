"""Shape extraction: the density field and the triangle mesh of a generator (applications/extract_mesh.py).

The script's three steps and what stands in for each here:

* ``get_sigma_field_np`` (extract_mesh.py:60-81) -> ``sigma_grid``: the backbone runs once, then ONE launch of the density lattice
  kernel (``p3d_sample_lattice``, csrc/shape.hip) fills the whole R^3 grid — instead of R^3 / 64^3 calls of ``G.sample_mixed`` that
  each rerun the backbone, send explicit coordinates, produce colour channels nobody reads and copy their block to the host;
* ``mcubes.marching_cubes`` (:89) -> ``marching_cubes``: the classify / scan / emit kernels on device tensors, a vectorised
  restatement on CPU tensors (the reference the kernels are tested against).  Both read the case table that mc_table.py generates;
  it is not Lorensen's table (ambiguous faces are resolved by separating their inside corners), so meshes are not comparable with
  PyMCubes' face for face;
* ``extract_geometry`` (:84-99) -> ``extract_geometry``: the two above and the script's rescale to world coordinates.

The per-vertex colour step (:198-215) needs nothing new: ``G.sample_mixed(vertices[None], None, ws, noise_mode='const')['rgb']``
already runs on the point kernel.
"""
import torch

from . import _lib, mc_table
from .training.triplane import _TriPlaneCore, frozen_pass
from .training.volumetric_rendering import renderer as _rmod

BLOCK_RESOLUTION = 64          # the script's block edge (extract_mesh.py:60)


def _axis(resolution, bound):
    """The lattice's coordinates along one axis, built as the script builds them (extract_mesh.py:64): fp32, on the CPU."""
    return torch.linspace(-bound, bound, resolution)


def _lattice_reason(G, ws):
    """None when sigma_grid can take the lattice kernel, else why not: the renderer's own conditions (``renderer.fallback_reason``) and, between them, the
    two that make ``G.sample_mixed`` something other than ``ImportanceRenderer.run_model`` on G's planes."""
    own = [(not isinstance(G, _TriPlaneCore) or type(G).sample_mixed is not _TriPlaneCore.sample_mixed, f'{type(G).__name__} samples through a sample_mixed of its own'),
           (type(G.renderer) is not _rmod.ImportanceRenderer, f'renderer {type(G.renderer).__name__} is not an ImportanceRenderer')]
    return _rmod.fallback_reason(_rmod.fused_policy, ws.is_cuda, G.rendering_kwargs, (G.decoder,), clamp_mode=False, own=own)


def _fallback_guard(ws, reason):
    _rmod._tensor_op_guard('sigma_grid', ws.is_cuda, reason, required='density lattice kernel required but unavailable',
                           instead='the block loop of G.sample_mixed, not the lattice kernel')


def _sigma_blocks(G, ws, axis, synthesis_kwargs):
    """get_sigma_field_np's loop (extract_mesh.py:66-79), for N images at once."""
    n, r = ws.shape[0], len(axis)
    out = torch.empty([n, r, r, r], dtype=torch.float32, device=ws.device)
    blocks = axis.split(BLOCK_RESOLUTION)
    b = BLOCK_RESOLUTION
    for xi, xs in enumerate(blocks):
        for yi, ys in enumerate(blocks):
            for zi, zs in enumerate(blocks):
                xx, yy, zz = torch.meshgrid(xs, ys, zs, indexing='ij')
                pts = torch.stack([xx, yy, zz], dim=-1).reshape(1, -1, 3).expand(n, -1, -1).to(ws.device)
                sigma = G.sample_mixed(pts, None, ws=ws, **synthesis_kwargs)['sigma']
                out[:, xi * b:xi * b + len(xs), yi * b:yi * b + len(ys), zi * b:zi * b + len(zs)] = sigma.reshape(n, len(xs), len(ys), len(zs))
    return out


@frozen_pass
def _planes(G, ws, **synthesis_kwargs):
    """The backbone pass G.sample_mixed makes (training/triplane.py:151-154), under the same frozen-pass rules."""
    return G._planes(ws, False, synthesis_kwargs)


@torch.no_grad()
def sigma_grid(G, ws, resolution=512, bound=None, **synthesis_kwargs):
    """get_sigma_field_np (extract_mesh.py:60-81) for ws [N, num_ws, w_dim]: the density at every point of the resolution^3 lattice
    linspace(-bound, bound, resolution)^3 as float32 [N, R, R, R] on ws's device, index (n, i, j, k) <-> point (x_i, y_j, z_k).
    ``bound`` defaults to box_warp / 2 and ``noise_mode`` to 'const', as in the script.

    Device tensors of a generator whose sample_mixed goes through ``ImportanceRenderer.run_model`` (TriPlaneGenerator, the
    conditional generators, ``_withBG``'s foreground) run the backbone once and one p3d_sample_lattice launch; CPU tensors and other
    generators take the script's own block loop through ``G.sample_mixed`` (on a device, under ``renderer.fused_policy``)."""
    if bound is None:
        bound = G.rendering_kwargs['box_warp'] * 0.5
    synthesis_kwargs.setdefault('noise_mode', 'const')
    axis = _axis(resolution, bound)
    reason = _lattice_reason(G, ws)
    if reason is not None:
        _fallback_guard(ws, reason)
        return _sigma_blocks(G, ws, axis, synthesis_kwargs)
    planes = _planes(G, ws, **synthesis_kwargs)
    return _rmod.fused_sample_lattice(planes, G.decoder, axis, axis, axis, G.rendering_kwargs)


# ---- marching cubes -----------------------------------------------------------------------------------------
_cpu_tables = None


def _tables():
    global _cpu_tables
    if _cpu_tables is None:
        tris = mc_table.triangles()
        count = torch.tensor([len(t) for t in tris], dtype=torch.int64)
        table = torch.full([256, 3 * mc_table.MAX_TRIANGLES], -1, dtype=torch.int64)
        for case, t in enumerate(tris):
            flat = [e for tri in t for e in tri]
            table[case, :len(flat)] = torch.tensor(flat, dtype=torch.int64)
        corner_off = torch.tensor([mc_table.CORNERS[c] for c, _ in mc_table.EDGES], dtype=torch.int64)     # [12, 3]
        axis = torch.tensor([a for _, a in mc_table.EDGES], dtype=torch.int64)
        _cpu_tables = count, table, corner_off, axis
    return _cpu_tables


def _marching_cubes_cpu(u, thr):
    X, Y, Z = u.shape
    count, table, corner_off, edge_axis = _tables()
    inside = u > thr
    crossed = torch.zeros([X, Y, Z, 3], dtype=torch.bool)
    crossed[:-1, :, :, 0] = inside[:-1] != inside[1:]
    crossed[:, :-1, :, 1] = inside[:, :-1] != inside[:, 1:]
    crossed[:, :, :-1, 2] = inside[:, :, :-1] != inside[:, :, 1:]
    idx = crossed.nonzero()                                    # [V, 4] = (i, j, k, axis): row-major corners, then axis
    i, j, k, a = idx.unbind(1)
    u0 = u[i, j, k]
    u1 = u[i + (a == 0).long(), j + (a == 1).long(), k + (a == 2).long()]
    t = (thr - u0) / (u1 - u0)
    vertices = idx[:, :3].to(torch.float32)
    rows = torch.arange(len(idx))
    vertices[rows, a] = vertices[rows, a] + t
    vid = torch.full([X, Y, Z, 3], -1, dtype=torch.int64)
    vid[crossed] = rows

    ins = inside.to(torch.int64)
    case = torch.zeros([X - 1, Y - 1, Z - 1], dtype=torch.int64)
    for c, (dx, dy, dz) in enumerate(mc_table.CORNERS):
        case |= ins[dx:X - 1 + dx, dy:Y - 1 + dy, dz:Z - 1 + dz] << c
    ntri = count[case]
    cubes = (ntri > 0).nonzero()                               # [A, 3], row-major
    cc = case[cubes.unbind(1)]
    edges = table[cc]                                          # [A, 3 * MAX_TRIANGLES], -1 beyond the case's triangles
    valid = torch.arange(edges.shape[1]) < 3 * count[cc].unsqueeze(1)
    e = edges.clamp(min=0)
    corner = cubes.unsqueeze(1) + corner_off[e]                # [A, 3 * MAX_TRIANGLES, 3]
    ids = vid[corner[..., 0], corner[..., 1], corner[..., 2], edge_axis[e]]
    faces = ids[valid].reshape(-1, 3)
    return vertices, faces


def _marching_cubes_device(u, thr):
    X, Y, Z = u.shape
    lib = _lib.lib()
    n = X * Y * Z
    blocks = int(lib.p3d_marching_cubes_blocks(X, Y, Z))
    dev = u.device
    mask = torch.empty([n], dtype=torch.uint8, device=dev)
    cases = torch.empty([n], dtype=torch.uint8, device=dev)
    counts = torch.empty([2, blocks], dtype=torch.int32, device=dev)
    stream = _lib.stream_of(u)
    _lib.check(lib.p3d_marching_cubes_classify(_lib.ptr(u), X, Y, Z, thr, _lib.ptr(mask), _lib.ptr(cases), _lib.ptr(counts), stream),
               'marching_cubes_classify')
    inclusive = torch.cumsum(counts, dim=1, dtype=torch.int64)
    offsets = (inclusive - counts).contiguous()
    n_vertices, n_faces = (int(v) for v in inclusive[:, -1].cpu())          # the one device-to-host copy: sizes the outputs
    vbase = torch.empty([n], dtype=torch.int32, device=dev)
    vertices = torch.empty([n_vertices, 3], dtype=torch.float32, device=dev)
    faces = torch.empty([n_faces, 3], dtype=torch.int64, device=dev)
    stream = _lib.stream_of(u)
    _lib.check(lib.p3d_marching_cubes_emit(_lib.ptr(u), X, Y, Z, thr, _lib.ptr(mask), _lib.ptr(cases), _lib.ptr(offsets[0]), _lib.ptr(offsets[1]),
                                           n_vertices, n_faces, _lib.ptr(vbase), _lib.ptr(vertices), _lib.ptr(faces), stream),
               'marching_cubes_emit')
    return vertices, faces


def marching_cubes(u, threshold):
    """mcubes.marching_cubes(u, threshold) as extract_mesh.py:89 uses it, on a float32 field u [X, Y, Z] (every dimension >= 2):
    (vertices float32 [V, 3] in index space, faces int64 [F, 3]) on u's device.  A corner is inside when u > threshold; the vertex of
    a crossed lattice edge sits at its lower corner plus t = (threshold - u_lower) / (u_upper - u_lower) along it, vertices are
    numbered by lower corner in row-major order, then by axis, faces come by cube in row-major order, then in case-table order, and
    (b - a) x (c - a) points from inside to outside (include/p3d_hip.h).  Device tensors run csrc/shape.hip's kernels and copy two
    totals to the host once (not graph-capturable); CPU tensors run the vectorised restatement."""
    if u.ndim != 3 or min(u.shape) < 2:
        raise ValueError(f'marching_cubes: u must be [X, Y, Z] with every dimension >= 2, got {tuple(u.shape)}')
    u = u.detach().to(torch.float32).contiguous()
    thr = float(torch.tensor(threshold, dtype=torch.float32))               # the fp32 threshold both paths compare and divide with
    if u.is_cuda:
        return _marching_cubes_device(u, thr)
    return _marching_cubes_cpu(u, torch.tensor(thr, dtype=torch.float32))


def extract_geometry(G, ws, resolution=512, threshold=50.0, **synthesis_kwargs):
    """extract_geometry (extract_mesh.py:84-99) for one image (ws [1, num_ws, w_dim]): the mesh of {sigma > threshold} over the cube
    [-box_warp/2, box_warp/2]^3 as (vertices float32 [V, 3] in world coordinates, faces int64 [F, 3]) on ws's device."""
    if ws.shape[0] != 1:
        raise ValueError(f'extract_geometry: one image at a time (ws has {ws.shape[0]})')
    bound = G.rendering_kwargs['box_warp'] * 0.5
    u = sigma_grid(G, ws, resolution, bound=bound, **synthesis_kwargs)[0]
    vertices, faces = marching_cubes(u, threshold)
    b_min, b_max = -bound, bound                                            # the script's rescale, in float64 (:93-96)
    vertices = (vertices.double() / (resolution - 1.0) * (b_max - b_min) + b_min).to(torch.float32)
    return vertices, faces
