"""csrc/bcast_ops.hip at the sizes training runs it: ``scale_channels``, ``fma.fma`` and the bias_act bias gradient against float64 CPU
autograd on the same dtype-rounded operands.

p3d_channel_dot (the style / demodulation gradients and, channels-last, every bias gradient) splits the H*W rows of an image into
clamp(ceil(rows / 256), 1, 256) chunks: col_dot_kernel writes one partial per chunk and col_dot_finish_kernel deals them round-robin
to eight lanes.  The cases give 1, 2, 255 and 256 chunks, rows per chunk that leave the 4-row unrolled loop a tail, column groups of
cpb = min(C / VEC, 32) that do not divide the 256 threads (C = 24 fp32, C = 96 fp16), a partial second column group (C = 160 fp32),
row_sum_cl_kernel with C / VEC not a power of two, the NCHW row path at n * C = 65535 (its last native size: bcast_fma_row_kernel's
grid y) and at 65536 (the tensor-op route), and the largest activation of a training step (the 512^2 SR layers: batch 4, 64 channels).

Bounds.  An element-wise result is one fp32 fma rounded once to the tensor dtype: |out - ref| <= u |ref| (u = 2^-24 fp32, 2^-11 fp16,
plus fp16's subnormal half-step), checked with no slack beyond 0.1 %.  A reduction accumulates in fp32: |out - ref| <= RED_TOL *
sum |terms| (+ u |ref| for the final rounding to the output dtype), so cancellation in the sum does not loosen the bar.  The bias
gradient is checked against the sum of the kernel's own dx, which is itself checked element-wise.  RED_TOL is about 3x the worst
measured on an MI355X (conftest.record_error): 6e-7, worst 1.9e-7 (the fma noise gradient of the NCHW 512^2 case; 1.1e-7 for the
style gradient at n * C = 65535).  Dropping one chunk of 1024 rows of a 512^2 image moves a sum by about 1e-4 of sum |terms|.
"""
import pytest
import torch

from conftest import record_error

pytestmark = pytest.mark.gpu

DT = {'f16': torch.float16, 'f32': torch.float32}
ULP = {torch.float16: (2.0 ** -11, 2.0 ** -25), torch.float32: (2.0 ** -24, 2.0 ** -150)}
RED_TOL = 6e-7

# (name, (N, C, H, W), layout, dtype)
CASES = [
    ('nhwc_1chunk_c24_f32', (2, 24, 16, 16), 'nhwc', 'f32'),
    ('nhwc_2chunks_c96_f16', (3, 96, 17, 17), 'nhwc', 'f16'),
    ('nhwc_255chunks_c160_f32', (1, 160, 255, 255), 'nhwc', 'f32'),
    ('nhwc_255chunks_c96_f16', (2, 96, 255, 255), 'nhwc', 'f16'),
    ('nhwc_256chunks_c24_f32', (2, 24, 256, 256), 'nhwc', 'f32'),
    ('nhwc_256chunks_c64_f16', (2, 64, 256, 256), 'nhwc', 'f16'),
    ('nhwc_c4_f32', (3, 4, 33, 31), 'nhwc', 'f32'),
    ('nhwc_c24_f16', (2, 24, 40, 9), 'nhwc', 'f16'),
    ('nhwc_512sq_b4_c64_f16', (4, 64, 512, 512), 'nhwc', 'f16'),
    ('nchw_c24_f32', (2, 24, 16, 16), 'nchw', 'f32'),
    ('nchw_c96_f16', (3, 96, 17, 24), 'nchw', 'f16'),
    ('nchw_512sq_b4_c32_f32', (4, 32, 512, 512), 'nchw', 'f32'),
    ('nchw_rows65535_f16', (3, 21845, 2, 4), 'nchw', 'f16'),
    ('nchw_rows65535_f32', (5, 13107, 1, 4), 'nchw', 'f32'),
    ('nchw_rows65536_f32', (2, 32768, 1, 4), 'nchw', 'f32'),
]


def _native(shape, layout):
    """Whether the native kernels take the tensor (bcast.layout: the NCHW row path indexes (n, c) rows with 16 bits)."""
    n, c, h, w = shape
    return layout == 'nhwc' or n * c < 65536


def _fmt(layout):
    return torch.channels_last if layout == 'nhwc' else torch.contiguous_format


def _seed(name):
    return sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) % 100003


def _elementwise(name, what, out, ref, roundings=1, scale=None):
    """max |out - ref| / (u |ref| + tiny): at most 1 for one correctly rounded result (``scale``: what stands for |ref|)."""
    u, tiny = ULP[out.dtype]
    r = ((out.detach().double().cpu() - ref).abs() / (u * (ref.abs() if scale is None else scale) + tiny)).max().item()
    record_error(f'bcast.{name}.{what}', r)
    print(f'{name:28s} {what:4s} {r:.3f} of one rounding')
    assert r <= 1.001 * roundings, (name, what, r)


def _reduction(name, what, out, ref, abs_sum):
    """max |out - ref| / (sum |terms|), after the final rounding to out's dtype is allowed for."""
    u, tiny = ULP[out.dtype]
    d = (out.detach().double().cpu() - ref).abs() - u * ref.abs() - tiny
    r = (d.clamp_min(0) / abs_sum.clamp_min(1e-300)).max().item()
    record_error(f'bcast.{name}.{what}', r)
    print(f'{name:28s} {what:4s} {r:.3e} of sum|terms|')
    assert r < RED_TOL, (name, what, r)


@pytest.mark.parametrize('name,shape,layout,dtype', CASES, ids=[c[0] for c in CASES])
def test_scale_channels_and_fma_at_size(hip_lib, name, shape, layout, dtype):
    from pix2pix3d_amd.torch_utils.ops import bcast, fma
    n, c, h, w = shape
    dt = DT[dtype]
    g = torch.Generator().manual_seed(_seed(name))
    x = torch.randn(shape, generator=g).to(dt)
    s = torch.randn(n, c, generator=g) + 1
    gy = torch.randn(shape, generator=g).to(dt)
    xd = x.cuda().contiguous(memory_format=_fmt(layout)).requires_grad_(True)
    gyd = gy.cuda().contiguous(memory_format=_fmt(layout))
    assert (bcast.layout(xd) is not None) == _native(shape, layout)

    # x * styles: y = x * s, gx = gy * s (element-wise), gs = sum_hw gy * x (p3d_channel_dot)
    c0 = dict(bcast.calls)
    sd = s.cuda().requires_grad_(True)
    y = bcast.scale_channels(xd, sd) if bcast.scale_channels_supported(xd, sd) else xd * sd.to(dt).reshape(n, c, 1, 1)
    gx, gs = torch.autograd.grad(y, [xd, sd], gyd)
    assert bcast.calls['dot'] - c0['dot'] == (1 if _native(shape, layout) else 0)
    xr, sr = x.double().requires_grad_(True), s.to(dt).double().requires_grad_(True)
    yr = xr * sr.reshape(n, c, 1, 1)
    gxr, gsr = torch.autograd.grad(yr, [xr, sr], gy.double())
    _elementwise(name, 'y', y, yr.detach())
    _elementwise(name, 'gx', gx, gxr)
    _reduction(name, 'gs', gs, gsr, (gy.double() * x.double()).abs().sum([2, 3]))
    del y, gx, gs, yr, gxr, gsr

    # fma(a, b, noise) as the unfused modulated conv uses it: b [N, C, 1, 1], the noise image per image and shared
    for shared in (False, True):
        tag = 'shared' if shared else 'per_image'
        b = (torch.rand(n, c, 1, 1, generator=g) + 0.5).to(dt)
        z = torch.randn(1 if shared else n, 1, h, w, generator=g).to(dt)
        bd, zd = b.cuda().requires_grad_(True), z.cuda().requires_grad_(True)
        c0 = dict(bcast.calls)
        out = fma.fma(xd, bd, zd)
        ga, gb, gz = torch.autograd.grad(out, [xd, bd, zd], gyd)
        assert bcast.calls['fma'] - c0['fma'] == (2 if _native(shape, layout) else 0)
        ar, br, zr = x.double().requires_grad_(True), b.double().requires_grad_(True), z.double().requires_grad_(True)
        outr = ar * br + zr
        gar, gbr, gzr = torch.autograd.grad(outr, [ar, br, zr], gy.double())
        if _native(shape, layout):
            _elementwise(name, f'fma.{tag}.y', out, outr.detach())
        else:                                                  # torch.addcmul: a product and a sum, each rounded
            _elementwise(name, f'fma.{tag}.y', out, outr.detach(), roundings=2, scale=(ar * br).detach().abs() + zr.detach().abs())
        _elementwise(name, f'fma.{tag}.ga', ga, gar)
        _reduction(name, f'fma.{tag}.gb', gb, gbr, (gy.double() * x.double()).abs().sum([2, 3], keepdim=True))
        _reduction(name, f'fma.{tag}.gz', gz, gzr, gy.double().abs().sum([0, 1] if shared else [1], keepdim=True))
        del out, ga, gb, gz, outr, gar, gbr, gzr


@pytest.mark.parametrize('name,shape,layout,dtype', CASES, ids=[c[0] for c in CASES])
def test_bias_gradient_at_size(hip_lib, name, shape, layout, dtype):
    """bias_act's db = dx summed over everything but the channel (channels-last: one [1, C] p3d_channel_dot over all N * H * W rows)."""
    from pix2pix3d_amd.torch_utils.ops import bcast, bias_act
    n, c, h, w = shape
    dt = DT[dtype]
    g = torch.Generator().manual_seed(_seed(name) + 7)
    x = torch.randn(shape, generator=g).to(dt)
    b = torch.randn(c, generator=g).to(dt)
    gy = torch.randn(shape, generator=g).to(dt)
    xd = x.cuda().contiguous(memory_format=_fmt(layout)).requires_grad_(True)
    bd = b.cuda().requires_grad_(True)
    c0 = dict(bcast.calls)
    y = bias_act.bias_act(xd, bd, act='lrelu')
    gx, gb = torch.autograd.grad(y, [xd, bd], gy.cuda().contiguous(memory_format=_fmt(layout)))
    assert bcast.calls['dot'] - c0['dot'] == (1 if _native(shape, layout) else 0)
    pre = x.double() + b.double().reshape(1, -1, 1, 1)
    slope = torch.where(pre > 0, 1.0, 0.2).double() * 2 ** 0.5
    ok = pre.abs() > 1e-3                                      # fp16 rounding of the pre-activation can take the other branch at 0
    gxr = gy.double() * slope
    _elementwise(name, 'dx', torch.where(ok.cuda(), gx, gxr.to(dt).cuda()), gxr, roundings=3)     # dy * alpha * gain, gain a C float: 1.82 measured
    gxk = gx.double().cpu()
    _reduction(name, 'db', gb, gxk.sum([0, 2, 3]), gxk.abs().sum([0, 2, 3]))
