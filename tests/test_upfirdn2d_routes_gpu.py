"""Every route of csrc/upfirdn2d.hip against the float64 oracle (oracle/ops_oracle.py: upfirdn2d, and upfirdn2d_grad for gradients), on
the case table of tests/upfirdn2d_routes.py: each tiled instantiation, the fused 4-tap channels-last kernel and the per-output
channels-last kernel (also on the same inputs, with P3D_UPFIRDN_NO_FIR4 in a child process), accumulate mode, each generic
specialisation, edge geometries, and the discriminator's and the Encoder's FIRs at the training sizes.

Inputs are rounded to the tensor dtype first; the oracle sees those values.  Forward and gradient errors are max|a - b| / max|b|
(conftest.rel_err); the adjoint check <A x, gy> = <x, A^T gy> on the kernel's own outputs is relative to the sum of |terms| of both
sides.  Every value is recorded through conftest.record_error.  Bounds are about 3x the worst measured on an MI355X (worst in brackets):
    forward, gradient  fp32 7e-7 (2.2e-7, cl_u1d1f4)   fp16 1.6e-3 (5.5e-4, the two fp16 passes of generic_sep4_down2)   fp64 1e-15 (3e-16)
    adjoint            fp32 1.5e-8 (4.7e-9)           fp16 1.5e-4 (4.6e-5, tiled_out1x17)                              fp64 6e-18 (1.7e-18)
One fp16 rounding of the output is up to 4.9e-4 of the range; the fp32 kernels differ from the oracle by the fp32 rounding of f * gain and
of the 16-term sum.
"""
import os
import re
import subprocess
import sys

import pytest
import torch

import upfirdn2d_routes as R
from conftest import ROOT, rel_err, record_error
from oracle import ops_oracle as O

pytestmark = pytest.mark.gpu

DT = {'f16': torch.float16, 'f32': torch.float32, 'f64': torch.float64}
TOL = {'f64': 1e-15, 'f32': 7e-7, 'f16': 1.6e-3}
ADJ_TOL = {'f64': 6e-18, 'f32': 1.5e-8, 'f16': 1.5e-4}


def _ops():
    from pix2pix3d_amd import _lib
    from pix2pix3d_amd.torch_utils.ops import upfirdn2d
    return _lib, upfirdn2d


def _seed(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003


def _kw(case):
    up, down, pad = R._geom(case)
    return dict(up=list(up), down=list(down), padding=list(pad), flip_filter=bool(case.flip), gain=float(case.gain))


def _fmt(t):
    """The memory format of a dense 4-D tensor (as the wrapper decides it)."""
    return torch.channels_last if t.stride(1) == 1 and t.shape[1] > 1 and not t.is_contiguous() else torch.contiguous_format


def _device(x, layout, offset=False):
    """x on the device in ``layout``; ``offset``: the same strides, one element past a 16-byte boundary."""
    if not offset:
        return x.cuda().contiguous(memory_format=torch.channels_last if layout == 'nhwc' else torch.contiguous_format)
    n, c, h, w = x.shape
    flat = torch.zeros(x.numel() + 8, dtype=x.dtype, device='cuda')
    v = flat[1:1 + x.numel()]
    v = v.view(n, c, h, w) if layout == 'nchw' else v.view(n, h, w, c).permute(0, 3, 1, 2)
    v.copy_(x)
    return v


def _inputs(case):
    g = torch.Generator().manual_seed(_seed(case.name))
    x = torch.randn(case.shape, generator=g).to(DT[case.dtype])
    f = R.make_filter(case.filt, _seed(case.name) + 1)
    xd = _device(x, case.layout, case.offset)
    assert xd.stride() == R.dense_strides(case.shape, case.layout) and (xd.data_ptr() % 16 == 0) == (not case.offset)
    return x, f, xd, None if f is None else torch.tensor(f, device='cuda')


def _record(case, what, err):
    route = '+'.join(R.wrapper_routes(case, no_fir4=None) if what != 'grad' else R.grad_routes(case, no_fir4=None))
    record_error(f'upfirdn2d.{case.name}.{route}.{what}', err)
    print(f'{case.name:34s} {route:48s} {what:5s} {err:.3e}')


def _check_forward(case):
    _lib, upfirdn2d = _ops()
    assert R.wrapper_routes(case) == case.routes
    x, f, xd, fd = _inputs(case)
    kw = _kw(case)
    n0 = _lib.launch_count('upfirdn2d')
    y = upfirdn2d.upfirdn2d(xd, fd, **kw)
    assert _lib.launch_count('upfirdn2d') - n0 == len(case.routes)
    yo = O.upfirdn2d(x.double().numpy(), f, **kw)
    out_layout = 'nhwc' if case.layout == 'nhwc' and case.shape[1] > 1 else 'nchw'
    assert tuple(y.shape) == yo.shape and y.dtype == xd.dtype and y.stride() == R.dense_strides(yo.shape, out_layout)
    err = rel_err(y.double().cpu().numpy(), yo)
    _record(case, 'fwd', err)
    assert err < TOL[case.dtype], (case.name, err)


def _check_gradient(case):
    """gx by autograd (the wrapper's backward: up and down exchanged, the filter mirrored) against the oracle's adjoint, and the adjoint
    identity on the kernel's own outputs."""
    _lib, upfirdn2d = _ops()
    x, f, xd, fd = _inputs(case)
    kw = _kw(case)
    xd.requires_grad_(True)
    y = upfirdn2d.upfirdn2d(xd, fd, **kw)
    g = torch.Generator().manual_seed(_seed(case.name) + 2)
    gy = torch.randn(y.shape, generator=g).to(y.dtype)
    gyd = gy.cuda().contiguous(memory_format=_fmt(y))
    n0 = _lib.launch_count('upfirdn2d')
    gx, = torch.autograd.grad(y, xd, gyd)
    assert _lib.launch_count('upfirdn2d') - n0 == len(R.grad_routes(case))
    gxo = O.upfirdn2d_grad(gy.double().numpy(), case.shape, f, **kw)
    err = rel_err(gx.double().cpu().numpy(), gxo)
    _record(case, 'grad', err)
    lhs, rhs = (y.detach().double() * gyd.double()), (xd.detach().double() * gx.double())
    adj = abs(lhs.sum().item() - rhs.sum().item()) / (lhs.abs().sum().item() + rhs.abs().sum().item())
    _record(case, 'adj', adj)
    assert err < TOL[case.dtype], (case.name, err)
    assert adj < ADJ_TOL[case.dtype], (case.name, adj)


@pytest.mark.parametrize('case', R.CASES, ids=[c.name for c in R.CASES])
def test_route_forward(hip_lib, case):
    _check_forward(case)


@pytest.mark.parametrize('case', R.CASES, ids=[c.name for c in R.CASES])
def test_route_gradient_and_adjoint(hip_lib, case):
    _check_gradient(case)


@pytest.mark.parametrize('name,dtype,shape', R.ACC_CASES, ids=[c[0] for c in R.ACC_CASES])
def test_accumulate_mode(hip_lib, name, dtype, shape):
    """upsample2d_add_: y = y0 + upsample2d(x, f) in one pass of the channels-last up = 2 kernel, y0 nonzero."""
    _lib, upfirdn2d = _ops()
    assert R.acc_route(dtype, shape) == 'cl<2,1,4>+acc'
    n, c, h, w = shape
    g = torch.Generator().manual_seed(_seed(name))
    x = torch.randn(shape, generator=g).to(DT[dtype])
    y0 = torch.randn(n, c, 2 * h, 2 * w, generator=g).to(DT[dtype])
    f = R.make_filter(('rand', 4, 4), _seed(name) + 1)
    xd, fd = _device(x, 'nhwc'), torch.tensor(f, device='cuda')
    y = _device(y0, 'nhwc')
    upfirdn2d.upsample2d_add_(y, xd, fd)
    ref = y0.double().numpy() + O.upfirdn2d(x.double().numpy(), f, up=2, padding=[2, 1, 2, 1], gain=4)
    err = rel_err(y.double().cpu().numpy(), ref)
    record_error(f'upfirdn2d.{name}.cl<2,1,4>+acc.fwd', err)
    print(f'{name:34s} cl<2,1,4>+acc fwd {err:.3e}')
    assert err < TOL[dtype], err
    # the same call through the C ABI must be taken (upsample2d_add_ falls back to two steps, silently, when it is declined)
    y2 = _device(y0, 'nhwc')
    code = _lib.lib().p3d_upfirdn2d_acc(
        _lib.ptr(xd), _lib.ptr(fd), _lib.ptr(y2), _lib.DTYPE_CODE[xd.dtype],
        _lib.i32x4(w, h, c, n), _lib.i64x4(xd.stride(3), xd.stride(2), xd.stride(1), xd.stride(0)),
        _lib.i32x2(4, 4), _lib.i64x2(fd.stride(1), fd.stride(0)),
        _lib.i32x4(2 * w, 2 * h, c, n), _lib.i64x4(y2.stride(3), y2.stride(2), y2.stride(1), y2.stride(0)),
        2, 2, 1, 1, 2, 2, 0, 4.0, _lib.stream_of(xd))
    assert code == _lib.P3D_OK and torch.equal(y2, y)


_production = {}


def _production_case(name):
    if not _production:
        _production.update((c.name, c) for c in R.production_cases())
    return _production[name]


@pytest.mark.parametrize('name', R.PRODUCTION, ids=R.PRODUCTION)
def test_production_size(hip_lib, name):
    """Batch 4 at 512^2 / 256^2: forward, gradient and adjoint."""
    case = _production_case(name)
    _check_forward(case)
    _check_gradient(case)


def test_u1d1f4_inputs_on_the_per_output_kernel(hip_lib):
    """The fused 4-tap cases again with P3D_UPFIRDN_NO_FIR4 set (read once per process, so in a child): the same inputs through
    upfirdn2d_cl_kernel<T, 1, 1, 4>, forward and gradient."""
    names = [c.name for c in R.CASES if c.routes == ['fir4']] + ['D_b512_blur_f16']
    expect = 2 * len(names) - 1                              # two tests per table case, one production test
    cmd = [sys.executable, '-m', 'pytest', '-q', '-s', '-p', 'no:cacheprovider', '-m', 'gpu', os.path.abspath(__file__),
           '-k', ' or '.join(names)]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, P3D_UPFIRDN_NO_FIR4='1'), stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=900)
    print(r.stdout[-6000:])
    assert r.returncode == 0, r.stdout[-4000:]
    assert f'{expect} passed' in r.stdout, r.stdout[-2000:]
    # the child's per-case lines (_record): every case ran on the per-output kernel; keep its values with this process's record
    seen = {}
    for line in r.stdout.splitlines():
        m = re.search(r'([A-Za-z]\w*)\s+(\S+)\s+(fwd|grad|adj)\s+(\S+)\s*$', line)         # (after pytest's progress dots)
        if m and m[1] in names:
            seen[(m[1], m[3])] = m[2]
            record_error(f'upfirdn2d.{m[1]}.{m[2]}.{m[3]}', float(m[4]))
    assert all(seen.get((n, w)) == 'cl<1,1,4>' for n in names for w in ('fwd', 'grad')), seen
