"""The weight gradient's host path (csrc/conv2d_grad.hip: WgradRequest -> plan_wgrad -> launch_wgrad_plan) against the answers the code gave BEFORE there was a plan.

tests/golden/wgrad_routes_parent.npz was recorded from the commit before this refactor (da17db4).  ``rows``: a scratch copy of that commit got a marker in front of
each of the thirteen launch sites of its ``bwd_weight_impl`` (= the p3d_wgrad_route code) and a dry run that takes the alignment facts and the workspace's bytes
instead of pointers; per row the marker (a negative status where the call is refused), the grid, ``ksplit``, ``chunks``, ``chunks_per_split``, ``psplit``,
``narrow_b``, ``xcd_pad`` and the reduce launch's ``nsplit`` it would have launched with, plus - from the UNMODIFIED parent library - p3d_conv2d_bwd_weight_workspace.
The rows are every 47th of the product  dtype {fp32, fp16, bf16x6} x channel pairs {3, 6, 32, 33, 40, 64, 128, 132, 200, 256, 512}^2 x small images {4x4, 20x36,
40x44, 24x128, 64x64, 256x256} x N {1, 4} x (k, stride, pad) {(3,1,1), (3,2,0), (1,1,0)} x the four alignment flag values x workspace {wanted, 2 x wanted, -1}
(47 shares no factor with any dimension: every value of every dimension stays), and every 1201st of the same product with the workspace one byte short, which is
the one refusal a sized request can meet.  ``switch_rows``: the rows ``switch_row_index`` of that table once more under each of the switches ``SWITCHES``, the dry
run and the unmodified library in fresh processes with that environment.  tests/golden/wgrad_errors.json: status and p3d_last_error() text of the unmodified
parent library for one call per argument check, each with exactly that fault.  tests/golden/wgrad_parent_digests.json: SHA-256 of ``gw`` from the parent's library
on the device for ``_CASES`` on the same CPU-seeded inputs (``P3D_WGRAD_NO_TR``: rows 1 and 3 in a process with that switch)."""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import pytest

from conftest import GOLDEN, ROOT, load_golden, rel_err

F32, F16, X6 = 0, 1, 4
SMALL_ALIGNED, BIG_ALIGNED = 1, 2
ROUTES = ['SKINNY_F16', 'SKINNY_F32', 'TR_SMALL_ROWK', 'TR_SMALL', 'TR_ROWK', 'TR', 'F16_SMALL', 'F16_FAST', 'F16_GENERAL', 'F32_SMALL', 'F32_X6', 'F32_FAST', 'F32_GENERAL']
R = {name: code for code, name in enumerate(ROUTES)}
SWITCH_ONLY = {R['F16_SMALL'], R['F16_FAST']}                  # fp16 register-transpose kernels: behind P3D_WGRAD_NO_TR / _NO_TR_SMALL
SWITCHES = [('P3D_WGRAD_NO_HALF', '1'), ('P3D_WGRAD_PLAN_OLD', '1'), ('P3D_WGRAD_WG_PER_CU', '3'), ('P3D_WGRAD_NO_SKINNY', '1'), ('P3D_WGRAD_NO_FAST', '1'),
            ('P3D_WGRAD_NO_SMALL', '1'), ('P3D_WGRAD_NO_TR', '1'), ('P3D_WGRAD_NO_TR_SMALL', '1')]
COLUMNS = ['dtype', 'n_img', 'small_h', 'small_w', 'c_small', 'big_h', 'big_w', 'c_big', 'kernel_size', 'stride', 'pad', 'flags', 'workspace_bytes',
           'route', 'grid', 'ksplit', 'chunks', 'chunks_per_split', 'psplit', 'narrow_b', 'xcd_pad', 'reduce_nsplit', 'workspace']
N_IN = 13                                                      # the first N_IN columns are the query's arguments
_I32, _I64 = ctypes.c_int32, ctypes.c_int64
_ROUTE_SIG = (ctypes.c_int, [ctypes.c_int] + [_I32] * 10 + [ctypes.c_uint32, _I64, ctypes.POINTER(_I32)])
_WORKSPACE_SIG = (_I64, [ctypes.c_int] + [_I32] * 6)


def _lib_handle():
    from pix2pix3d_amd import _lib
    from pix2pix3d_amd.torch_utils.ops import conv2d_gradfix      # noqa: F401  (registers the signatures)
    return _lib.lib()


def _answers(h, args):
    """[route, the eight plan numbers, p3d_conv2d_bwd_weight_workspace] of one row's arguments."""
    plan = (_I32 * 8)()
    route = h.p3d_conv2d_bwd_weight_route(*args, plan)
    assert h.p3d_conv2d_bwd_weight_route(*args, None) == route
    dt, n, hs, ws, cs, hb, wb, cb, k = args[:9]
    return [route] + list(plan) + [h.p3d_conv2d_bwd_weight_workspace(dt, n, hs, ws, cs, cb, k)]


def test_plan_gives_the_routes_of_the_interleaved_code_it_replaces():
    h = _lib_handle()
    g = load_golden('wgrad_routes_parent')
    assert g['columns'].tolist() == COLUMNS
    rows = g['rows'].tolist()
    seen = {r[N_IN] for r in rows}
    assert len(rows) >= 3000 and seen >= set(range(13)) - SWITCH_ONLY and not seen & SWITCH_ONLY and min(seen) < 0
    for r in rows:
        assert _answers(h, r[:N_IN]) == r[N_IN:], r


def _switch_child_rows():
    g = load_golden('wgrad_routes_parent')
    rows = g['rows'].tolist()
    return [rows[i][:N_IN] for i in g['switch_row_index'].tolist()]


def _switch_child():
    """(fresh process, host only, no torch) the answers for the fixed rows under this process's environment, as one JSON line."""
    h = ctypes.CDLL(os.path.join(ROOT, 'pix2pix3d_amd', 'libp3d_hip.so'))
    h.p3d_conv2d_bwd_weight_route.restype, h.p3d_conv2d_bwd_weight_route.argtypes = _ROUTE_SIG
    h.p3d_conv2d_bwd_weight_workspace.restype, h.p3d_conv2d_bwd_weight_workspace.argtypes = _WORKSPACE_SIG
    print(json.dumps([_answers(h, a) for a in _switch_child_rows()]))


def _clean_env(**extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith('P3D_WGRAD_')}
    env.update(extra)
    return env


@pytest.mark.parametrize('switch', range(len(SWITCHES)), ids=[s[0] for s in SWITCHES])
def test_each_switch_keeps_its_meaning(switch):
    """The switches are read once per process: one fresh child per switch answers the fixed rows; the golden section was recorded the same way."""
    g = load_golden('wgrad_routes_parent')
    assert g['switches'].tolist() == [s[0] for s in SWITCHES] and 36 <= len(g['switch_row_index']) <= 48
    want = g['switch_rows'][switch].tolist()
    name, value = SWITCHES[switch]
    out = subprocess.run([sys.executable, os.path.abspath(__file__), 'switch-child'], env=_clean_env(**{name: value}), capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    assert json.loads(out.stdout.strip().splitlines()[-1]) == want


def test_all_thirteen_routes_are_pinned():
    g = load_golden('wgrad_routes_parent')
    seen = {r[N_IN] for r in g['rows'].tolist()} | {r[0] for s in g['switch_rows'].tolist() for r in s}
    assert seen >= set(range(13))
    no_tr = {r[0] for r in g['switch_rows'][[s[0] for s in SWITCHES].index('P3D_WGRAD_NO_TR')].tolist()}
    assert no_tr >= SWITCH_ONLY


# ---- one call per argument check, with exactly that fault ------------------------------------------------------------------------------------------------------
P = 16          # a dummy non-null, 16-byte aligned pointer: every call below is refused before anything is launched
_BASE = dict(small_img=P, big_img=P, gw=P, workspace=P, workspace_bytes='wanted', dtype=F32, n_img=1, small_h=16, small_w=16, c_small=64, big_h=16, big_w=16, c_big=64,
             kernel_size=3, stride=1, pad=1)
_FAULTS = [dict(small_img=None), dict(big_img=None), dict(gw=None), dict(workspace=None), dict(dtype=2), dict(dtype=3), dict(n_img=0), dict(kernel_size=2), dict(stride=3),
           dict(pad=2), dict(workspace_bytes='one byte short'), dict(workspace=24)]
_ENTRY_FAULTS = [('p3d_conv2d_bwd_weight', f) for f in _FAULTS] + [('p3d_conv2d_bwd_weight_scaled', f) for f in (_FAULTS[2], _FAULTS[4], _FAULTS[6], _FAULTS[10], _FAULTS[11])]


def _faulty_call(h, entry, fault):
    args = dict(_BASE)
    assert set(fault) <= set(args)
    wanted = h.p3d_conv2d_bwd_weight_workspace(F32, args['n_img'], args['small_h'], args['small_w'], args['c_small'], args['c_big'], args['kernel_size'])
    args.update(fault)
    args['workspace_bytes'] = wanted - (args['workspace_bytes'] == 'one byte short')
    tail = (1.0, None) if entry.endswith('_scaled') else (None,)
    code = getattr(h, entry)(*args.values(), *tail)
    return int(code), h.p3d_last_error().decode()


def test_every_argument_check_answers_as_it_did():
    h = _lib_handle()
    with open(os.path.join(GOLDEN, 'wgrad_errors.json')) as f:
        want = json.load(f)
    assert len(want) == len(_ENTRY_FAULTS)
    for (entry, fault), row in zip(_ENTRY_FAULTS, want):
        assert row['entry'] == entry and row['fault'] == fault and row['code'] in (-1, -2), row
        assert _faulty_call(h, entry, fault) == (row['code'], row['text']), row
    assert len({row['text'] for row in want}) >= 6      # (one call per distinct check, not one check many times)


# ---- on the device: the plan is what is launched ----------------------------------------------------------------------------------------------------------------
# tests/test_conv_grad_gpu.py's bars, relative to the output's maximum, against an fp64 sum over the same values
_TOL = {F32: 2e-5, F16: 4e-3, X6: 4e-6}
_CASES = [      # id, dtype, N, HS, WS, Cs, HB, WB, Cb, k, stride, pad, route
    ('tr_small_rowk', F16, 1, 48, 128, 64, 48, 128, 64, 3, 1, 1, 'TR_SMALL_ROWK'),       # chunks_per_split 2, 48 splits
    ('tr_small', F16, 3, 20, 36, 64, 20, 36, 32, 3, 1, 1, 'TR_SMALL'),
    ('tr_rowk', F16, 1, 16, 64, 64, 33, 129, 128, 3, 2, 0, 'TR_ROWK'),                   # psplit 2, stride 2
    ('tr', F16, 1, 12, 20, 128, 12, 20, 128, 3, 1, 1, 'TR'),
    ('f16_general', F16, 2, 4, 4, 40, 4, 4, 33, 3, 1, 1, 'F16_GENERAL'),
    ('f32_small', F32, 1, 12, 20, 64, 12, 20, 64, 3, 1, 1, 'F32_SMALL'),
    ('f32_x6', X6, 1, 9, 11, 136, 9, 11, 132, 3, 1, 1, 'F32_X6'),
    ('f32_fast', F32, 1, 12, 20, 64, 12, 20, 128, 3, 1, 1, 'F32_FAST'),                  # psplit 2
    ('f32_general', F32, 2, 4, 4, 40, 4, 4, 33, 3, 1, 1, 'F32_GENERAL'),
    ('skinny_few_small', F16, 2, 24, 24, 3, 24, 24, 128, 1, 1, 0, 'SKINNY_F16'),
    ('skinny_few_big', F32, 2, 24, 24, 64, 24, 24, 6, 1, 1, 0, 'SKINNY_F32'),
]
_NO_TR_CASES = {0: 'F16_SMALL', 2: 'F16_FAST'}                  # rows of _CASES that reach the register-transpose fp16 kernels under P3D_WGRAD_NO_TR


def _planned_route(h, case):
    dt, n, hs, ws, cs, hb, wb, cb, k, stride, pad = case[1:12]
    plan = (_I32 * 8)()
    return h.p3d_conv2d_bwd_weight_route(dt, n, hs, ws, cs, hb, wb, cb, k, stride, pad, SMALL_ALIGNED | BIG_ALIGNED, -1, plan), list(plan)


@pytest.mark.parametrize('case', _CASES, ids=[c[0] for c in _CASES])
def test_suggested_shapes_plan_the_route_they_are_meant_to_reach(case):
    """(host) the device test's shapes against the plan, so that a geometry that no longer reaches its kernel fails here and not silently there."""
    route, plan = _planned_route(_lib_handle(), case)
    assert route == R[case[12]]
    assert plan[7] > 1          # more than one partial tile to sum


def _digests():
    with open(os.path.join(GOLDEN, 'wgrad_parent_digests.json')) as f:
        return json.load(f)


def _run_on_device(h, case, want_route=None, want_digest=None):
    """One weight gradient on the device: two launches, twice the same bits, the sum an fp64 CPU evaluation gives; returns SHA-256 of gw's bytes."""
    import torch
    from pix2pix3d_amd import _lib
    name, dt, n, hs, ws, cs, hb, wb, cb, k, stride, pad = case[:12]
    if want_route is not None:
        assert _planned_route(h, case)[0] == R[want_route]
    tdt = torch.float16 if dt == F16 else torch.float32
    g = torch.Generator().manual_seed(1000 + [c[0] for c in _CASES].index(name))
    small = torch.randn(n, hs, ws, cs, generator=g).to(tdt)
    big = torch.randn(n, hb, wb, cb, generator=g).to(tdt)
    bp = torch.nn.functional.pad(big.double(), (0, 0, pad, pad + 2, pad, pad + 2))
    sd = small.double()
    ref = torch.stack([torch.stack([torch.einsum('nijs,nijb->sb', sd, bp[:, ky:ky + (hs - 1) * stride + 1:stride, kx:kx + (ws - 1) * stride + 1:stride])
                                    for kx in range(k)], -1) for ky in range(k)], -2)
    sdev, bdev = small.cuda(), big.cuda()
    nbytes = int(h.p3d_conv2d_bwd_weight_workspace(dt, n, hs, ws, cs, cb, k))
    work = torch.empty(nbytes // 4, dtype=torch.float32, device='cuda')
    out = []
    for _ in range(2):
        gw = torch.zeros(cs, cb, k, k, dtype=tdt, device='cuda')
        before = _lib.launch_count('conv')
        _lib.check(h.p3d_conv2d_bwd_weight(_lib.ptr(sdev), _lib.ptr(bdev), _lib.ptr(gw), _lib.ptr(work), nbytes, dt, n, hs, ws, cs, hb, wb, cb, k, stride, pad,
                                           _lib.stream_of(gw)), name)
        assert _lib.launch_count('conv') - before == 2
        out.append(gw.cpu())
    assert torch.equal(out[0], out[1])
    e = rel_err(out[0].double().numpy(), ref.numpy())
    digest = hashlib.sha256(out[0].numpy().tobytes()).hexdigest()
    print(name, 'workspace', nbytes, 'rel err', e, digest)
    assert e < _TOL[dt], e
    if want_digest is not None:
        assert digest == want_digest, 'gw differs in its bytes from what the parent commit computed'
    return digest


@pytest.mark.gpu
@pytest.mark.parametrize('case', _CASES, ids=[c[0] for c in _CASES])
def test_the_planned_route_is_what_is_launched(hip_lib, case):
    """One geometry per route of the default environment: the plan names the route, the call makes two launches, and gw is bit for bit what the parent commit gave."""
    _run_on_device(_lib_handle(), case, want_route=case[12], want_digest=_digests()['default'][case[0]])


def _no_tr_child():
    h = _lib_handle()
    want = _digests()['P3D_WGRAD_NO_TR']
    for i, route in _NO_TR_CASES.items():
        _run_on_device(h, _CASES[i], want_route=route, want_digest=want[_CASES[i][0]])


@pytest.mark.gpu
def test_register_transpose_fp16_kernels_behind_their_switch(hip_lib):
    """conv_wgrad_kernel<__half, 128, true, true> and <__half, 64, true> run only with P3D_WGRAD_NO_TR (read once per process): one fresh child, same assertions."""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), 'no-tr-child'], env=_clean_env(P3D_WGRAD_NO_TR='1'), capture_output=True, text=True, timeout=240)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-4000:]


if __name__ == '__main__':
    {'switch-child': _switch_child, 'no-tr-child': _no_tr_child}[sys.argv[1]]()
