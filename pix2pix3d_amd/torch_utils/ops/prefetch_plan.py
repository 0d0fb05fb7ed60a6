"""The prefetch plan of device inference: what was issued ahead on a device's side stream (every layer's styles and pre-modulated weights,
networks_stylegan2.prefetch_styles) and which of it the consuming streams already wait behind.  One ``PrefetchPlan`` per device (modconv.plan_for).
Written against the little it needs of streams and events — ``current_stream()``, ``stream.wait_event(event)`` / ``wait_stream(side)``, ``stream.cuda_stream`` (hashable;
unique within ONE device: the map of waited positions is per plan), ``new_event()`` / ``event.record(stream)`` — so it runs on the CPU with stand-ins (tests/test_prefetch_plan.py)."""
import collections

# What one layer finds planned: its styles, (pre-modulated weights, route tag) or None, the event / position on the side stream behind which both exist, its plan
Entry = collections.namedtuple('Entry', 'styles pre event pos plan')


class PrefetchPlan:
    entries = {}             # id(layer) -> Entry, ONE table for every device (a layer lives on one): "is anything planned at all?" stays one truth test per layer call

    def __init__(self, side, current_stream, new_event):
        self.side, self.current_stream, self.new_event = side, current_stream, new_event
        self.seq = 0             # position of the newest event on the side stream (monotonic for the life of the process: a later position implies every earlier one)
        self.latest = None       # (event, position) of that newest event
        self.own_until = 0       # waits for positions up to this one are for the entry's OWN event (a network's first layer, then its ToRGB group); later ones for everything issued
        self.waited = {}         # consuming stream -> the position it already waits behind
        self.ahead = {}          # id(network) -> (the ws it was planned for, the plan's keys): plans issued ahead of a network that runs later in the step
        self.deferred = []       # callables that issue such plans, run once the current network's own plan is out (run_deferred)

    def issue(self, own):
        """Record an event on the side stream behind everything launched there so far -> (event, position).  ``own``: consumers wait for THIS event rather than
        for the newest one (a network's first layer must not stand behind every modulation of the step); plans issued ahead never move that mark."""
        ev = self.new_event()
        ev.record(self.side)
        self.seq += 1
        self.latest = (ev, self.seq)
        if own:
            self.own_until = self.seq
        return self.latest

    def add(self, layer, styles, pre, mark):
        self.entries[id(layer)] = Entry(styles, pre, mark[0], mark[1], self)
        return id(layer)

    def enter(self, records, products, rgb_products, ahead):
        """Enter a network's layers behind the events they wait for -> their keys.  records: (layer, styles) in forward order; products: per record (product, did
        making it launch anything?), consumed as the marks are set — a generator's launches land right in front of their layer's mark; rgb_products(): called once,
        right behind the first mark — {record index: (product, launched?)} of the ToRGB group.
        One mark per layer that LAUNCHED something; a layer that did not (a shared-weight layer after the first) shares the mark of the last one that did (take
        skips a position its stream already waits behind).  Right behind the FIRST layer's mark: every ToRGB layer's weight modulation (3-6 us each, eleven per
        step, otherwise in line in front of their layers) and one mark for all that launched one — the network's first layer does not stand behind them, its
        first ToRGB (tens of microseconds later) waits for that one mark, and from there on a wait is for everything issued."""
        mark, rgb_pre, keys = None, {}, []
        for k, ((layer, styles), (pre, fresh)) in enumerate(zip(records, products)):
            if fresh or mark is None:
                first = mark is None
                mark = self.issue(own=first and not ahead)
                if first:
                    rgb_pre = rgb_products()
                    rgb_mark = self.issue(own=not ahead) if any(launched for _, launched in rgb_pre.values()) else mark
            keys.append(self.add(layer, styles, rgb_pre[k][0], rgb_mark) if k in rgb_pre else self.add(layer, styles, pre, mark))
        return keys

    @classmethod
    def take(cls, layer, elision=True, wait_latest=True):
        """Pop this layer's Entry and make the current stream wait for it — unless (``elision``) the stream already waits behind its position: in the captured
        step every wait is an edge between two branches of the graph, idle device in front of the layer's first kernel whether or not the event fired long ago
        (27 per step, 5.8 us each: profiles/round5_u_step_trace.txt; A/B +0.4 ... +1.1 %, profiles/round6_a_*).  A wait for a position past ``own_until`` is
        (``wait_latest``) for the NEWEST event: by then the side stream has long run dry, so a network costs three edges and the heads planned ahead none."""
        e = cls.entries.pop(id(layer), None)
        if e is None:
            return None
        self, cur = e.plan, e.plan.current_stream()
        if not elision or e.pos > self.waited.get(cur.cuda_stream, -1):
            ev, pos = self.latest if elision and wait_latest and e.pos > self.own_until else (e.event, e.pos)
            cur.wait_event(ev)
            self.waited[cur.cuda_stream] = pos
        return e

    def joined(self, stream):
        """True when ``stream`` already waits behind everything on the side stream."""
        return self.latest is not None and self.waited.get(stream.cuda_stream, -1) >= self.latest[1]

    @classmethod
    def drop(cls, keys):
        """Forget these entries (an interrupted forward's must never reach the next one; a plan made for another latent tensor)."""
        for k in keys:
            cls.entries.pop(k, None)

    def finish(self, keys, elision=True):
        """End of the network's forward: the current stream joins the side stream (no further edge if it already stands behind its newest event)."""
        main = self.current_stream()
        if not (elision and self.joined(main)):
            main.wait_stream(self.side)
        self.drop(keys)

    def defer(self, hook):
        self.deferred.append(hook)

    def run_deferred(self, run=True):
        """Issue the plans of the networks later in the step: behind the current one on the side stream, before any of its tensors is released."""
        hooks, self.deferred = self.deferred, []
        for hook in hooks if run else ():
            hook()

    def hand_over(self, network, ws, keys):
        self.ahead[id(network)] = (ws, keys)

    def claim(self, network, ws):
        """The keys of the plan issued ahead for ``network`` with this very ``ws``, else None (a plan for another tensor is dropped)."""
        ws_planned, keys = self.ahead.pop(id(network), (None, ()))
        if ws_planned is ws:
            return keys
        self.drop(keys)
