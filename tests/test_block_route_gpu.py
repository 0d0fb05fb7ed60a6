"""The synthesis pass on the device does, call for call, what it did before SynthesisBlock's forms were decided by modconv.block_route: every C ABI call with its
scalars and stream (the prefetch stream's launches included — a premodulation nobody takes, or an in-line one the plan used to cover, is a difference), the
cross-stream waits, the launch wrappers and the SplitActs in their order, and bit-identical outputs (tests/golden/block_routes.json, recorded from the parent
commit by tests/golden/make_block_routes_golden.py)."""
import pytest

import block_trace as T

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize('case_id', list(T.cases()))
def test_trace_and_digests_equal_the_parents(hip_lib, case_id):
    rec = T.load_recording()
    want, stored = T.recorded_events(rec, case_id), rec['cases'][case_id]
    events, (first, second) = T.run_case(T.cases()[case_id])
    for k, (a, b) in enumerate(zip(events, want)):
        assert a == b, (k, a, b, [T.arg_names(a[1]) if a[0] == 'call' else None])
    assert len(events) == len(want)
    for runs in (first, second):
        assert {k: v for k, v in runs.items() if k not in stored['unstable']} == stored['digests']


def test_an_orig_backbone_plans_what_its_forward_takes(hip_lib):
    """architecture='orig': the only ToRGB is the last block's, and no skip image reaches it — the plan must see that block as the forward does (block_route with
    has_img=False: the streaming ToRGB, which modulates in-kernel) and make no ToRGB product; every 3x3 layer's product comes from the plan, none is made in line."""
    import torch
    from pix2pix3d_amd.torch_utils.ops import modconv
    from pix2pix3d_amd.training.networks_stylegan2 import SynthesisNetwork
    torch.manual_seed(0)
    net = SynthesisNetwork(w_dim=64, img_resolution=256, img_channels=3, channel_max=128, architecture='orig').cuda().eval().requires_grad_(False)
    ws = torch.randn(1, net.num_ws, 64, device='cuda')

    def once():
        with T.Tracer() as t, torch.no_grad():
            img = net(ws, noise_mode='none')
        torch.cuda.synchronize()
        return t.events, img
    once()
    events, img = once()
    taps = T.arg_names('p3d_modulate_weights').index('taps')
    made = [(ev[2], ev[3][taps]) for ev in events if ev[:2] == ['call', 'p3d_modulate_weights']]
    assert made == [('side', 9)] * 13, made                      # conv1 of b4, conv0 + conv1 of b8 .. b256
    assert [ev[1] for ev in events if ev[0] == 'wrapper'] == ['torgb']
    saved, modconv.prefetch_styles = modconv.prefetch_styles, False
    try:
        assert torch.equal(once()[1], img)
    finally:
        modconv.prefetch_styles = saved
