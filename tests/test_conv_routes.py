"""The forward convolution's host path (csrc/conv2d.hip: ConvRequest -> plan_conv -> launch_conv_plan) against the answers the code gave BEFORE there was a plan.

tests/golden/conv_routes_parent.npz was recorded from the commit before this refactor (eda3cb0).  ``rows``: a scratch copy of that commit got a marker in front of
every launch site of its ``conv2d_nhwc_run_io`` / ``launch_conv`` and a dry run that could be told "no workspace", "y misaligned", "has out_scale / in_scale"; per
row the marker (= the p3d_conv_route code; a negative status where the call is refused), the split-K scratch bytes it asked for and the ``y_split`` it stored, plus —
from the UNMODIFIED parent library, for the rows those entry points can express — the answers of p3d_conv2d_nhwc_workspace and p3d_conv2d_nhwc_bf16x3_io_plan.
``forward_workspace_rows``: p3d_conv2d_forward_workspace of the unmodified parent library.  tests/golden/conv_forward_errors.json: status and p3d_last_error() text of
the unmodified parent library for one call per argument check of the forward entry points, each with exactly that fault (``_BASE`` below + the row's overrides)."""
import ctypes
import json
import os
import threading

import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, load_golden, rel_err

F32, F16, BF3, X6 = 0, 1, 3, 4
HAS_OUT_SCALE, HAS_IN_SCALE, HAS_WORKSPACE, Y_ALIGNED = 1, 2, 4, 8
GENERIC, GENERIC_SPLITK, HALO, HALO_X6P, H2_F16, R2_BF16X3, CONVT_H2_F16 = range(7)


def _lib_handle():
    from pix2pix3d_amd import _lib
    from pix2pix3d_amd.torch_utils.ops import conv2d_gradfix, modconv      # noqa: F401  (register the signatures)
    return _lib.lib()


def _golden(name):
    with open(os.path.join(GOLDEN, name + '.json')) as f:
        return json.load(f)


class _x6_presplit:
    """P3D_X6_PRESPLIT for the duration of a block (the one switch the library reads at every call); restored afterwards."""

    def __enter__(self):
        self.prev = os.environ.get('P3D_X6_PRESPLIT')
        return self

    def set(self, v):
        if v is None or v < 0:
            os.environ.pop('P3D_X6_PRESPLIT', None)
        else:
            os.environ['P3D_X6_PRESPLIT'] = str(v)

    def __exit__(self, *exc):
        self.set(None)
        if self.prev is not None:
            os.environ['P3D_X6_PRESPLIT'] = self.prev


def test_plan_gives_the_routes_of_the_interleaved_code_it_replaces():
    h = _lib_handle()
    g = load_golden('conv_routes_parent')
    assert g['columns'].tolist() == ['dtype', 'n_img', 'h', 'wdt', 'ci', 'co', 'per_image_weights', 'kernel_size', 'resample', 'x_split', 'y_split', 'flags', 'x6_presplit',
                            'route', 'scratch_bytes', 'y_split_stored', 'nhwc_workspace', 'io_plan', 'io_plan_bytes']
    rows = g['rows'].tolist()
    assert len(rows) >= 3000 and {r[13] for r in rows} == {-2, -1, 0, 1, 2, 3, 4, 5, 6}
    n_ws = n_plan = 0
    with _x6_presplit() as env:
        for r in rows:
            dt, n, hh, w, ci, co, per, k, res, xs, ys, flags, x6, route, nbytes, ys_stored, ws, plan, plan_bytes = r
            env.set(x6)
            stride = co * k * k * ci if per else 0
            got = ctypes.c_int64(-1)
            assert h.p3d_conv2d_nhwc_route(dt, n, hh, w, ci, co, stride, k, res, xs, ys, flags, ctypes.byref(got)) == route, r
            assert got.value == nbytes, r
            assert h.p3d_conv2d_nhwc_route(dt, n, hh, w, ci, co, stride, k, res, xs, ys, flags, None) == route, r
            if ws >= 0:                    # plain operands, a workspace: what p3d_conv2d_nhwc_workspace assumes
                n_ws += 1
                assert h.p3d_conv2d_nhwc_workspace(dt, n, hh, w, ci, co, stride, k, res) == ws == (nbytes if route >= 0 else 0), r
            if plan != -9:                 # ... and p3d_conv2d_nhwc_bf16x3_io_plan, which falls back to a plain result where a split one is refused
                n_plan += 1
                assert h.p3d_conv2d_nhwc_bf16x3_io_plan(n, hh, w, ci, co, stride, k, res, xs, ys, ctypes.byref(got)) == plan, r
                assert got.value == plan_bytes, r
                assert route < 0 or (plan == ys and (ys_stored != 0) == bool(ys) and plan_bytes == nbytes), r
    assert n_ws > 1000 and n_plan > 400, (n_ws, n_plan)


def test_forward_workspace_gives_the_answers_of_the_dry_run_it_replaces():
    h = _lib_handle()
    g = load_golden('conv_routes_parent')
    assert g['forward_workspace_columns'].tolist() == ['dtype', 'n_img', 'h', 'wdt', 'ci', 'co', 'kernel_size', 'stride', 'transposed', 'bytes']
    rows = g['forward_workspace_rows'].tolist()
    assert len(rows) > 1000 and sum(1 for r in rows if r[-1] > 0) > 300
    assert any(r[6] == 1 and r[-1] == 0 for r in rows) and {(r[7], r[8]) for r in rows if r[-1] > 0} == {(1, 0), (1, 1), (2, 0), (2, 1)}
    for r in rows:
        assert h.p3d_conv2d_forward_workspace(*r[:-1]) == r[-1], r


# ---- one call per argument check, with exactly that fault ------------------------------------------------------------------------------------------------------
P = 16          # a dummy non-null, 16-byte aligned pointer: every call below is refused before anything is launched
_NHWC = dict(x=P, w=P, y=P, dtype=F32, bias=None, noise=None, noise_strength=None, zeros128=P, n_img=1, h=16, wdt=16, ci=64, co=64, w_img_stride=0, kernel_size=3, resample=0,
             act=0, gain=1.0, clamp=-1.0)
_WS = dict(workspace=None, workspace_bytes=0, stream=None)
_BASE = {      # entry point -> a valid call's arguments, in the order of its signature
    'p3d_conv2d_nhwc': dict(_NHWC, stream=None),
    'p3d_conv2d_nhwc_ws': dict(_NHWC, **_WS),
    'p3d_conv2d_nhwc_bf16x3_io': dict({k: v for k, v in _NHWC.items() if k != 'dtype'}, x_split=0, y_split=0, **_WS),
    'p3d_conv2d_nhwc_scaled': dict(x=P, w=P, y=P, dtype=F32, out_scale=P, **{k: v for k, v in _NHWC.items() if k not in ('x', 'w', 'y', 'dtype')}, **_WS),
    'p3d_conv2d_nhwc_scaled_in': dict(x=P, w=P, y=P, dtype=BF3, in_scale=P, out_scale=P, **{k: v for k, v in _NHWC.items() if k not in ('x', 'w', 'y', 'dtype')}, **_WS),
    'p3d_conv2d_nhwc_bf16x3_io_plan': dict(n_img=1, h=16, wdt=16, ci=64, co=64, w_img_stride=0, kernel_size=3, resample=0, x_split=0, want_y_split=0, workspace_bytes='int64*'),
    'p3d_conv3x3_torgb_f16': dict(x=P, w=P, y=P, bias=None, zeros128=P, rgb_w=P, rgb_bias=None, rgb_out=P, rgb_co=3, rgb_clamp=256.0, n_img=1, h=32, wdt=32, ci=64, co=128,
                                  w_img_stride=0, act=1, gain=1.0, clamp=-1.0, stream=None),
    'p3d_conv3x3_torgb_split': dict(x_split=P, w_split=P, bias=None, noise=None, noise_strength=None, zeros128=P, rgb_wmod_split=P, rgb_bias=None, img_nhwc=P, prev_nhwc=None,
                                    f4x4_host=None, rgb_co=32, rgb_clamp=256.0, n_img=12, h=64, wdt=64, ci=64, co=128, w_img_stride=0, act=1, gain=1.0, clamp=-1.0, stream=None),
    'p3d_conv2d_forward': dict(x=P, weight=P, y=P, w_scratch=P, zeros128=P, dtype=F32, n_img=1, h=16, wdt=16, ci=64, co=64, kernel_size=3, stride=1, transposed=0, out_h=0, out_w=0,
                               **_WS),
    'p3d_conv2d_bwd_data': dict(gy=P, weight=P, gx=P, w_scratch=P, zeros128=P, dtype=F32, n_img=1, gy_h=16, gy_w=16, ci=64, co=64, kernel_size=3, stride=1, transposed=0, x_h=16,
                                x_w=16, **_WS),
}
_FAULTS = [    # (entry point, the one thing wrong with the call)
    ('p3d_conv2d_nhwc', dict(resample=3)), ('p3d_conv2d_nhwc', dict(x=None)), ('p3d_conv2d_nhwc', dict(zeros128=None)), ('p3d_conv2d_nhwc', dict(n_img=0)),
    ('p3d_conv2d_nhwc', dict(co=0)), ('p3d_conv2d_nhwc', dict(dtype=2)), ('p3d_conv2d_nhwc', dict(kernel_size=5)), ('p3d_conv2d_nhwc', dict(kernel_size=1, resample=1)),
    ('p3d_conv2d_nhwc', dict(ci=48)), ('p3d_conv2d_nhwc', dict(dtype=F16, ci=32)), ('p3d_conv2d_nhwc', dict(x=24)), ('p3d_conv2d_nhwc', dict(w=8)),
    ('p3d_conv2d_nhwc', dict(resample=2, h=2)), ('p3d_conv2d_nhwc', dict(resample=1, bias=P)), ('p3d_conv2d_nhwc', dict(resample=1, act=1)),
    ('p3d_conv2d_nhwc_ws', dict(y=None)), ('p3d_conv2d_nhwc_ws', dict(ci=48)),
    ('p3d_conv2d_nhwc_scaled', dict(dtype=F16)), ('p3d_conv2d_nhwc_scaled', dict(wdt=0)),
    ('p3d_conv2d_nhwc_bf16x3_io', dict(y_split=1, co=80)), ('p3d_conv2d_nhwc_bf16x3_io', dict(y_split=1, resample=2)), ('p3d_conv2d_nhwc_bf16x3_io', dict(y_split=1, h=4)),
    ('p3d_conv2d_nhwc_bf16x3_io', dict(y_split=1, resample=1)), ('p3d_conv2d_nhwc_bf16x3_io', dict(x_split=1, w=None)),
    ('p3d_conv2d_nhwc_scaled_in', dict(in_scale=None)), ('p3d_conv2d_nhwc_scaled_in', dict(out_scale=None)), ('p3d_conv2d_nhwc_scaled_in', dict(dtype=F32)),
    ('p3d_conv2d_nhwc_scaled_in', dict(in_scale=24)), ('p3d_conv2d_nhwc_scaled_in', dict(n_img=8, h=4, wdt=4, ci=512, co=512)), ('p3d_conv2d_nhwc_scaled_in', dict(x=None)),
    ('p3d_conv2d_nhwc_bf16x3_io_plan', dict(workspace_bytes=None)), ('p3d_conv2d_nhwc_bf16x3_io_plan', dict(ci=48)), ('p3d_conv2d_nhwc_bf16x3_io_plan', dict(resample=3)),
    ('p3d_conv2d_nhwc_bf16x3_io_plan', dict(want_y_split=1, resample=2, h=2)),
    ('p3d_conv3x3_torgb_f16', dict(x=None)), ('p3d_conv3x3_torgb_f16', dict(rgb_co=9)), ('p3d_conv3x3_torgb_f16', dict(act=2)), ('p3d_conv3x3_torgb_f16', dict(co=64)),
    ('p3d_conv3x3_torgb_f16', dict(h=16)), ('p3d_conv3x3_torgb_f16', dict(y=24)), ('p3d_conv3x3_torgb_f16', dict(x=24)),
    ('p3d_conv3x3_torgb_split', dict(img_nhwc=None)), ('p3d_conv3x3_torgb_split', dict(prev_nhwc=P)), ('p3d_conv3x3_torgb_split', dict(noise=P)),
    ('p3d_conv3x3_torgb_split', dict(act=2)), ('p3d_conv3x3_torgb_split', dict(n_img=0)), ('p3d_conv3x3_torgb_split', dict(co=256)), ('p3d_conv3x3_torgb_split', dict(n_img=11)),
    ('p3d_conv3x3_torgb_split', dict(rgb_co=48)), ('p3d_conv3x3_torgb_split', dict(x_split=24)),
    ('p3d_conv2d_forward', dict(x=None)), ('p3d_conv2d_forward', dict(dtype=2)), ('p3d_conv2d_forward', dict(ci=0)), ('p3d_conv2d_forward', dict(kernel_size=1, stride=2)),
    ('p3d_conv2d_forward', dict(kernel_size=1, ci=1000, co=24)), ('p3d_conv2d_forward', dict(w_scratch=None)), ('p3d_conv2d_forward', dict(zeros128=None)),
    ('p3d_conv2d_forward', dict(ci=48)), ('p3d_conv2d_forward', dict(dtype=F16, ci=32, co=128, h=32, wdt=32, transposed=1, stride=1)),
    ('p3d_conv2d_bwd_data', dict(gy=None)), ('p3d_conv2d_bwd_data', dict(co=48)), ('p3d_conv2d_bwd_data', dict(kernel_size=2)),
]


def _faulty_call(h, entry, fault):
    """(status, message) of ``entry`` called with ``_BASE[entry]`` + ``fault``."""
    args = dict(_BASE[entry])
    assert set(fault) <= set(args)
    args.update(fault)
    keep = ctypes.c_int64(0)
    code = getattr(h, entry)(*[ctypes.byref(keep) if v == 'int64*' else v for v in args.values()])
    return int(code), h.p3d_last_error().decode()


def test_every_argument_check_answers_as_it_did():
    h = _lib_handle()
    want = _golden('conv_forward_errors')
    assert len(want) == len(_FAULTS)
    texts = set()
    for (entry, fault), row in zip(_FAULTS, want):
        assert row['entry'] == entry and row['fault'] == fault and row['code'] in (-1, -2), row
        assert _faulty_call(h, entry, fault) == (row['code'], row['text']), row
        texts.add(row['text'])
    assert len(texts) >= 40      # (one call per distinct check, not one check many times)


# ---- on the device: the plan is what is launched ----------------------------------------------------------------------------------------------------------------
# tests/test_conv_gpu.py's bars, relative to the output's maximum, against fp64 convolutions of the same operands: exact fp32 1e-5 (2e-5 for its 512-channel layers,
# K = 4608: test_lowres_512_channel_layers_take_the_split_k_schedule), fp16 2e-3, bf16x3 1e-5, bf16x6 3e-6
_TOL = {F32: 1e-5, F16: 2e-3, BF3: 1e-5, X6: 3e-6}
_TOL_F32_512 = 2e-5
_CASES = [      # id, dtype, ci, co, h, w, n_img, kernel, resample, x_split, workspace?, P3D_X6_PRESPLIT, route
    ('generic_1x1', F32, 64, 96, 16, 16, 2, 1, 0, 0, True, None, GENERIC),
    ('splitk_512_with_workspace', F32, 512, 512, 16, 16, 1, 3, 0, 0, True, None, GENERIC_SPLITK),
    ('halo_512_without_workspace', F32, 512, 512, 16, 16, 1, 3, 0, 0, False, None, HALO),
    ('x6p_forced', X6, 64, 64, 16, 16, 2, 3, 0, 0, False, 2, HALO_X6P),
    ('h2_f16', F16, 128, 128, 32, 32, 8, 3, 0, 0, False, None, H2_F16),
    ('r2_split_in', BF3, 32, 128, 64, 64, 12, 3, 0, 1, True, None, R2_BF16X3),
    ('convT_h2_f16', F16, 64, 128, 32, 32, 2, 3, 1, 0, True, None, CONVT_H2_F16),
]


def _case_flags(ws):
    return Y_ALIGNED | (HAS_WORKSPACE if ws else 0)


@pytest.mark.parametrize('case', _CASES, ids=[c[0] for c in _CASES])
def test_suggested_shapes_plan_the_route_they_are_meant_to_reach(case):
    """(host) the device test's shapes against the plan, so that a geometry that no longer reaches its kernel fails here and not silently there."""
    _, dt, ci, co, hh, w, n, k, res, xs, ws, x6, route = case
    h = _lib_handle()
    with _x6_presplit() as env:
        env.set(x6)
        nbytes = ctypes.c_int64(-1)
        assert h.p3d_conv2d_nhwc_route(dt, n, hh, w, ci, co, co * k * k * ci, k, res, xs, 0, _case_flags(ws), ctypes.byref(nbytes)) == route
        assert (nbytes.value > 0) == (route == GENERIC_SPLITK) or not ws


def _split_storage(v):
    """fp32 [N,C,H,W] -> fp32-typed channels-last storage of [32 x bf16 hi | 32 x bf16 lo] rows (tests/test_split_acts.py)."""
    n, c, h, w = v.shape
    x = v.permute(0, 2, 3, 1).reshape(n, h, w, c // 32, 32)
    hi = x.to(torch.bfloat16)
    lo = (x - hi.float()).to(torch.bfloat16)
    return torch.stack([hi, lo], dim=-2).reshape(n, h, w, c // 32, 64).view(torch.float32).reshape(n, h, w, c).permute(0, 3, 1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize('case', _CASES, ids=[c[0] for c in _CASES])
def test_the_planned_route_is_what_is_launched(hip_lib, case):
    """One geometry per route code: the conv family's launch counter moves by 2 where the plan deals the K loop out (kernel + epilogue) and by 1 otherwise, and
    the result is the convolution."""
    from pix2pix3d_amd import _lib
    from pix2pix3d_amd.torch_utils.ops import modconv
    _, dt, ci, co, hh, w, n, k, res, xs, ws, x6, route = case
    h = _lib.lib()
    torch.manual_seed(ci + co + hh)
    tdt = torch.float16 if dt == F16 else torch.float32
    x = torch.randn(n, ci, hh, w, device='cuda').to(tdt).contiguous(memory_format=torch.channels_last)
    weight, styles = torch.randn(co, ci, k, k, device='cuda'), torch.randn(n, ci, device='cuda') + 1
    wmod = modconv.modulate_weights(weight, styles, demodulate=(k == 3), dtype=modconv.BF16X3 if dt == BF3 else tdt)
    wref = wmod if dt != BF3 else modconv.modulate_weights(weight, styles, demodulate=(k == 3), dtype=torch.float32)
    wq = wref.double().reshape(n, co, k, k, ci).permute(0, 1, 4, 2, 3).cpu()
    xd = x.double().cpu()
    if res == 1:
        ref = torch.stack([F.conv_transpose2d(xd[i:i + 1], wq[i].transpose(0, 1), stride=2)[0] for i in range(n)])
    else:
        ref = torch.stack([F.conv2d(xd[i:i + 1], wq[i], padding=k // 2)[0] for i in range(n)])
    xin = _split_storage(x.cpu()).contiguous(memory_format=torch.channels_last).cuda() if xs else x
    y = torch.empty(list(ref.shape), dtype=tdt, device='cuda').contiguous(memory_format=torch.channels_last)
    stride = co * k * k * ci
    with _x6_presplit() as env:
        env.set(x6)
        nbytes = ctypes.c_int64(0)
        assert h.p3d_conv2d_nhwc_route(dt, n, hh, w, ci, co, stride, k, res, xs, 0, _case_flags(ws), ctypes.byref(nbytes)) == route
        assert (nbytes.value > 0) == (route == GENERIC_SPLITK) or not ws
        work = torch.empty([nbytes.value // 4], dtype=torch.float32, device='cuda') if ws and nbytes.value > 0 else None
        geo = (_lib.ptr(modconv._zeros_page(x.device)), n, hh, w, ci, co, stride, k, res, 0, 1.0, -1.0)
        tail = (_lib.ptr(work), nbytes.value if work is not None else 0, _lib.stream_of(x))
        before = _lib.launch_count('conv')
        if dt == BF3:
            code = h.p3d_conv2d_nhwc_bf16x3_io(_lib.ptr(xin), _lib.ptr(wmod), _lib.ptr(y), None, None, None, *geo, xs, 0, *tail)
        else:
            code = h.p3d_conv2d_nhwc_ws(_lib.ptr(xin), _lib.ptr(wmod), _lib.ptr(y), dt, None, None, None, *geo, *tail)
        _lib.check(code, case[0])
        assert _lib.launch_count('conv') - before == (2 if route == GENERIC_SPLITK else 1)
    e = rel_err(y.double().cpu().numpy(), ref.numpy())
    print(case[0], e)
    assert e < (_TOL_F32_512 if (dt, ci) == (F32, 512) else _TOL[dt]), e


@pytest.mark.gpu
def test_both_scales_from_two_host_threads_in_turn(hip_lib):
    """The shared-weight form (in_scale = the styles, out_scale = the demodulation) called from two host threads one after the other gives what one thread gives:
    the input scale travels in the request, not in per-thread state."""
    from pix2pix3d_amd.torch_utils.ops import modconv
    torch.manual_seed(7)
    n, ci, co, res = 2, 64, 64, 16
    x = torch.randn(n, ci, res, res, device='cuda').contiguous(memory_format=torch.channels_last)
    weight, styles = torch.randn(co, ci, 3, 3, device='cuda'), torch.randn(n, ci, device='cuda') + 1
    w1 = modconv.modulate_weights(weight, torch.ones(1, ci, device='cuda'), demodulate=False, dtype=modconv.BF16X3)
    d = modconv.demod_coefs(weight, styles)
    run = lambda: modconv.conv2d(x, w1, split=True, in_scale=styles, out_scale=d)
    y0 = run()
    wq = modconv.modulate_weights(weight, styles, dtype=torch.float32).double().reshape(n, co, 3, 3, ci).permute(0, 1, 4, 2, 3).cpu()
    ref = torch.stack([F.conv2d(x[i:i + 1].double().cpu(), wq[i], padding=1)[0] for i in range(n)])
    assert rel_err(y0.double().cpu().numpy(), ref.numpy()) < _TOL[BF3]
    got = []

    def worker():
        torch.cuda.set_device(x.device)
        got.append(run())
        torch.cuda.synchronize()

    for _ in range(2):
        t = threading.Thread(target=worker)
        t.start()
        t.join()
    assert len(got) == 2 and torch.equal(got[0], y0) and torch.equal(got[1], y0)
