"""The position logic of the prefetch plan (torch_utils/ops/prefetch_plan.py) on the CPU, with stand-in streams and events: how many cross-stream waits a
network's forward makes (the counts tests/test_model_gpu.py::test_prefetch_plan_waits_are_few_and_change_nothing pins on the device), and that two devices'
plans never see each other's events."""
from pix2pix3d_amd.torch_utils.ops.prefetch_plan import PrefetchPlan


class Event:
    def record(self, stream):
        self.stream = stream


class Stream:
    def __init__(self, device, handle=0):
        self.device, self.cuda_stream, self.waits, self.joins = device, handle, [], []      # (handle 0: the default stream of EVERY device)

    def wait_event(self, ev):
        self.waits.append(ev)

    def wait_stream(self, st):
        self.joins.append(st)


class Layer:
    pass


class Device:
    def __init__(self, name):
        self.main, self.side = Stream(name), Stream(name, 7)
        self.plan = PrefetchPlan(self.side, lambda: self.main, Event)


def issue(plan, layers, rgb, ahead=False, fresh=None):
    """PrefetchPlan.enter — the loop prefetch_styles itself runs — over stand-in layers: a mark behind the first layer's work (the network's own), one behind
    the ToRGB group's weight modulations, then one per layer that launched something (``fresh``: all but the ToRGB layers and the shared-weight layers after the first)."""
    launched = [(None, layer not in rgb and (fresh is None or fresh[k])) for k, layer in enumerate(layers)]
    return plan.enter([(layer, ('styles', layer)) for layer in layers], launched, lambda: {k: (None, True) for k, layer in enumerate(layers) if layer in rgb}, ahead)


def network(n_blocks):
    """conv0, conv1, torgb per block — in the order prefetch_styles plans them and the forward takes them."""
    layers = [Layer() for _ in range(3 * n_blocks)]
    return layers, set(layers[2::3])


def forward(layers, **switches):
    for layer in layers:
        e = PrefetchPlan.take(layer, **switches)
        assert e is not None and e.styles == ('styles', layer) and e.pre is None


def test_a_network_costs_three_waits_and_a_network_planned_ahead_none():
    dev = Device('gpu0')
    backbone, heads = network(7), [network(2), network(2)]
    keys = issue(dev.plan, *backbone, fresh=[k not in (1, 3, 4) for k in range(21)])
    dev.plan.defer(lambda: [dev.plan.hand_over(h[0][0], 'ws', issue(dev.plan, *h, ahead=True)) for h in heads])
    dev.plan.run_deferred()
    forward(backbone[0])
    assert 2 <= len(dev.main.waits) <= 3                        # its first layer, its ToRGB group, everything issued
    assert dev.plan.joined(dev.main)
    dev.plan.finish(keys)
    assert dev.main.joins == []                                 # already behind the side stream's newest event: no further edge
    for h in heads:
        head_keys = dev.plan.claim(h[0][0], 'ws')
        assert head_keys is not None
        forward(h[0])
        dev.plan.finish(head_keys)
    assert len(dev.main.waits) <= 3 and dev.main.joins == [] and not PrefetchPlan.entries
    assert all(ev.stream is dev.side for ev in dev.main.waits)


def test_without_elision_every_layer_waits_for_its_own_event():
    dev = Device('gpu0')
    layers, rgb = network(7)
    keys = issue(dev.plan, layers, rgb)
    forward(layers, elision=False)
    assert len(dev.main.waits) == len(layers)
    dev.plan.finish(keys, elision=False)
    assert dev.main.joins == [dev.side] and not PrefetchPlan.entries
    # ... and with elision but without the "everything issued" rule: one wait per distinct event, each for the layer's own
    layers, rgb = network(7)
    before = len(dev.main.waits)
    issue(dev.plan, layers, rgb)
    forward(layers, wait_latest=False)
    assert len(dev.main.waits) - before == len(layers) - len(rgb)       # (the ToRGB group's event lies before the second layer's)


def test_two_devices_interleaved_never_meet():
    a, b = Device('gpu0'), Device('gpu1')
    assert a.main.cuda_stream == b.main.cuda_stream             # the collision the per-device map of waited positions exists for
    (la, ra), (lb, rb) = network(5), network(5)
    cur = {}
    a.plan.current_stream = b.plan.current_stream = lambda: cur['stream']      # ONE notion of "the current stream", as in a process that switches devices
    keys_a = issue(a.plan, la, ra)
    keys_b = issue(b.plan, lb, rb)
    for x, y in zip(la, lb):
        for dev, other, layer in ((a, b, x), (b, a, y)):
            cur['stream'], others = dev.main, (dict(other.plan.waited), list(other.main.waits))
            assert PrefetchPlan.take(layer).plan is dev.plan
            assert all(ev.stream is dev.side for ev in dev.main.waits)
            assert (other.plan.waited, other.main.waits) == others      # what the other device's stream stands behind is untouched
    assert len(a.main.waits) == len(b.main.waits) == 2          # (first layer; conv1 -> everything issued) on each: none elided on the strength of the other's positions
    # a stream is joined by its OWN device's events only: b issues more, a's stream — same handle — stays joined to a's plan and b's is not
    issue(b.plan, *network(1))
    assert a.plan.joined(a.main) and not b.plan.joined(b.main)
    for dev, keys in ((a, keys_a), (b, keys_b)):
        cur['stream'] = dev.main
        dev.plan.finish(keys)
    assert a.main.joins == [] and b.main.joins == [b.side]
    PrefetchPlan.entries.clear()


def test_entries_of_an_interrupted_forward_never_reach_the_next():
    dev = Device('gpu0')
    layers, rgb = network(3)
    issue(dev.plan, layers, rgb)
    forward(layers[:4])                                         # ... and the forward raises here
    PrefetchPlan.drop(id(layer) for layer in layers)           # the next forward's first act (prefetch_styles), whether or not it plans again
    assert not PrefetchPlan.entries and all(PrefetchPlan.take(layer) is None for layer in layers)
    # a plan handed over for another latent tensor is dropped, not picked up
    dev.plan.hand_over(layers[0], 'ws', issue(dev.plan, layers, rgb, ahead=True))
    assert dev.plan.claim(layers[0], 'other ws') is None and not PrefetchPlan.entries and dev.plan.claim(layers[0], 'ws') is None
