"""CPU: the filter store of hip_ops (filter_lookup, filters_after_update, refresh_module_filters, the registry of constant weights)
against the transcription of the functions it replaced (tests/filter_store_ref.py).

Both run in this process on the same host tensors.  Only what touches the process is replaced, by the same fakes on both sides: the
single-layer and the many-layer launch (they return numbered tensors and write (timer name, kind, the weights, the wanted directions)
into a trace), the device test, the capture query and the stream query.  Seeded random sequences of updates, lookups, in-place changes,
registrations, refreshes and switches of capture / stream / PREPACK drive both; after every operation the traces, what each lookup
returned, every module's cache, the plan, the prepacked filters and the constant registry are the same.  The events the sequences must
reach are counted in the transcription."""
import random
import time
import types

import pytest
import torch

from meta_interpolation_amd import _hip, hip_ops
from tests import filter_store_ref as ref

TIMER = {"convk": "convk_filters", "wino": "conv3x3_filters", "wino2": "conv3x3_filters"}
UPDATES = {"4d": [(8, 4, 3, 3), (8,), (8, 8, 3, 3), (8,)], "5d": [(2, 8, 4, 5, 5), (2, 8), (2, 8, 8, 3, 3)]}
MODULES = [(8, 4, 3, 3), (8, 8, 3, 3), (8, 4, 5, 5)]
CONSTS = [(2, 8, 8, 3, 3), (8, 8, 3, 3), (2, 8, 4, 5, 5)]
SEEDS, OPS = 50, 300
EVENTS = ["module_hit", "module_eviction", "module_remake_for_direction", "prepacked_hit", "prepacked_miss_by_version", "const_hit",
          "const_make", "plan_learned", "plan_refused_for_another_kind", "refresh_launched", "lookup_while_capturing", "update_with_prepack_off"]


class Side:
    """The fakes of one side: its trace and the serial numbers of the tensors its launches return."""

    def __init__(self):
        self.trace, self.serial = [], 0

    def _tensor(self, want):
        if not want:
            return None
        self.serial += 1
        return torch.tensor([self.serial])

    @staticmethod
    def _name(w):                  # a weight by what a launch reads of it (refresh hands a detached alias of the module's weight)
        return (w.data_ptr(), w._version, tuple(w.shape))

    def single(self, kind, weight, fwd, bwd):
        self.trace.append((TIMER[kind], kind, self._name(weight), (bool(fwd), bool(bwd))))
        return self._tensor(fwd), self._tensor(bwd)

    def multi(self, kind, jobs):
        if not jobs:
            return []
        self.trace.append((TIMER[kind] + "_multi", kind, tuple(self._name(w) for w, _, _ in jobs), tuple((bool(f), bool(b)) for _, f, b in jobs)))
        return [(self._tensor(f), self._tensor(b)) for _, f, b in jobs]


class World:
    capturing, stream = False, 11


def _serials(pair):
    return None if pair is None else tuple(None if t is None else int(t[0]) for t in pair)


@pytest.fixture
def sides(monkeypatch):
    """(world, the transcription's side, hip_ops's side), both stores empty and on the fakes."""
    world, old, new = World(), Side(), Side()
    for name, value in dict(is_cuda=lambda t: True, capturing=lambda: world.capturing, current_stream=lambda: world.stream,
                            launch_single=lambda timer, kind, w, f, b: old.single(kind, w, f, b), launch_multi=old.multi,
                            workspace_floats=hip_ops._workspace_floats, PREPACK=True, _pack_plans={}, _last_update=None, _prepacked={},
                            _const_weights={}).items():
        monkeypatch.setattr(ref, name, value)
    for name, value in dict(_on_device=lambda t: True, _capturing=lambda: world.capturing, _raw_stream=lambda: world.stream,
                            _make_filters=new.single, _filters_multi=new.multi, PREPACK=True, _pack_plans={}, _last_update=None,
                            _prepacked={}, _const_weights={}).items():
        monkeypatch.setattr(hip_ops, name, value)
    monkeypatch.setattr(_hip, "require_cuda", lambda *tensors: None)        # (the device test of the public functions)
    return world, old, new


def _same_state(old, new, mods, where):
    assert old.trace == new.trace, where
    for r, n in mods:
        assert list(r._filters) == list(n._filters), where
        assert [_serials(v) for v in r._filters.values()] == [_serials(v) for v in n._filters.values()], where
    assert ref._pack_plans == hip_ops._pack_plans, where
    assert list(ref._prepacked) == list(hip_ops._prepacked), where
    assert [(v[1], _serials(v[2:])) for v in ref._prepacked.values()] == [(v[1], _serials(v[2:])) for v in hip_ops._prepacked.values()], where
    assert list(ref._const_weights) == list(hip_ops._const_weights), where
    held = lambda store: [(e[1], [(k, _serials(v)) for k, v in e[2].items()]) for e in store.values()]
    assert held(ref._const_weights) == held(hip_ops._const_weights), where
    assert (ref._last_update is None) == (hip_ops._last_update is None), where
    if ref._last_update is not None:
        assert ref._last_update[:2] == hip_ops._last_update[:2] and all(a is b for a, b in zip(ref._last_update[2], hip_ops._last_update[2])), where


def _drive(seed, world, old, new):
    rnd = random.Random(seed)
    mods = [(types.SimpleNamespace(weight=w, _filters={}), types.SimpleNamespace(weight=w, _filters={}))
            for w in (torch.zeros(s) for s in MODULES)]
    consts = [torch.zeros(s) for s in CONSTS]
    updates = []                    # the outputs of the last two updates
    for step in range(OPS):
        where = "seed %d operation %d" % (seed, step)
        op = rnd.choices(["lookup", "update", "bump", "register", "refresh", "switch"], [55, 12, 8, 8, 7, 10])[0]
        if op == "update":
            outs = [torch.zeros(s) for s in UPDATES[rnd.choice(sorted(UPDATES))]]
            if rnd.random() < 0.1:
                outs = []
            updates = (updates + [outs])[-2:]
            ref.filters_after_update(outs)
            hip_ops.filters_after_update(outs)
        elif op == "lookup":
            source = rnd.choice(["module", "module", "module-no-cache", "const", "update", "update", "update", "fresh"])
            caches = (None, None)
            if source.startswith("module"):
                r, n = rnd.choice(mods)
                w = r.weight
                if source == "module":
                    caches = (r._filters, n._filters)
            elif source == "const":
                w = rnd.choice(consts)
            elif source == "update":
                pool = [o for outs in updates for o in outs if o.dim() >= 4]
                w = rnd.choice(pool) if pool else torch.zeros(8, 8, 3, 3)
            else:
                w = torch.zeros(rnd.choice(MODULES + CONSTS))
            kind = rnd.choice(["convk", "wino", "wino2"]) if w.shape[-1] == 3 else "convk"
            fwd, bwd = rnd.choice([(True, False), (False, True), (True, True), (True, True)])
            if caches[0] is None and rnd.random() < 0.5:        # the public functions: the lookup without a module's cache
                if kind == "convk":
                    got = ref.convk_filters(w, fwd, bwd), hip_ops.convk_filters(w, fwd, bwd)
                else:
                    got = ref.conv3x3_filters(w, fwd, bwd, f2=kind == "wino2"), hip_ops.conv3x3_filters(w, fwd, bwd, f2=kind == "wino2")
            else:
                got = ref._filters(kind, w, fwd, bwd, caches[0]), hip_ops.filter_lookup(kind, w, fwd, bwd, caches[1])
            assert _serials(got[0]) == _serials(got[1]), where
            assert tuple(t is not None for t in got[1]) == (fwd, bwd), where
        elif op == "bump":
            pool = [r.weight for r, _ in mods] + consts + [o for outs in updates for o in outs]
            rnd.choice(pool).add_(1.0)
        elif op == "register":
            w = rnd.choice(consts)
            register = rnd.random() < 0.7
            for store in (ref, hip_ops):
                (store.register_const_weight if register else store.unregister_const_weight)(w)
        elif op == "refresh":
            ref.refresh_module_filters([r for r, _ in mods])
            hip_ops.refresh_module_filters([n for _, n in mods])
        else:
            what = rnd.choice(["capture", "stream", "prepack"])
            if what == "capture":
                world.capturing = rnd.random() < 0.4
            elif what == "stream":
                world.stream = rnd.choice([11, 22])
            else:
                ref.PREPACK = hip_ops.PREPACK = rnd.random() < 0.75
        _same_state(old, new, mods, where + " (" + op + ")")
    world.capturing, world.stream = False, 11
    ref.PREPACK = hip_ops.PREPACK = True


def test_random_sequences_leave_the_same_launches_results_and_stores_as_the_transcription(sides):
    world, old, new = sides
    ref.EVENTS.clear()
    launches, timers = 0, set()
    for seed in range(SEEDS):
        for store in (ref, hip_ops):
            store._pack_plans.clear(), store._prepacked.clear(), store._const_weights.clear()
            store._last_update = None
        launches += len(old.trace)
        timers |= {(e[0], e[1]) for e in old.trace}
        old.trace.clear(), new.trace.clear()
        _drive(seed, world, old, new)
    launches += len(old.trace)
    timers |= {(e[0], e[1]) for e in old.trace}
    print("launches %d; events %s" % (launches, dict(ref.EVENTS)))
    assert launches > SEEDS * OPS // 10
    for name in EVENTS:
        assert ref.EVENTS[name] >= 1, (name, dict(ref.EVENTS))
    assert timers == {(TIMER[kind] + multi, kind) for kind in TIMER for multi in ("", "_multi")}


def test_the_sixty_fifth_constant_weight_puts_the_oldest_out(sides):
    world, old, new = sides
    ws = [torch.zeros(8, 8, 3, 3) for _ in range(ref._CONST_WEIGHTS_MAX + 1)]
    assert hip_ops._CONST_WEIGHTS_MAX == ref._CONST_WEIGHTS_MAX == 64
    for store in (ref, hip_ops):
        for w in ws[:-1]:
            assert store.register_const_weight(w) is w
        store.convk_filters(ws[0], True, True)
        store.convk_filters(ws[1], True, False)
    assert len(old.trace) == 2 and list(hip_ops._const_weights) == [w.data_ptr() for w in ws[:-1]]
    for store in (ref, hip_ops):
        store.register_const_weight(ws[-1])
    assert list(ref._const_weights) == list(hip_ops._const_weights) == [w.data_ptr() for w in ws[1:]]
    for store in (ref, hip_ops):
        store.convk_filters(ws[0], True, True)          # no longer a constant: made again, and again
        store.convk_filters(ws[0], True, True)
        store.convk_filters(ws[1], True, True)          # still one: only the missing direction is made
        store.convk_filters(ws[1], True, True)
    assert old.trace == new.trace and len(old.trace) == 5 and old.trace[-1][3] == (False, True)
    _same_state(old, new, [], "after the eviction")


def test_the_kind_table_keeps_timer_names_and_entry_points():
    lib = _hip.lib()
    assert list(hip_ops._KINDS) == ["convk", "wino", "wino2"]               # the order of the many-layer launches
    for kind, k in hip_ops._KINDS.items():
        assert k.timer == TIMER[kind] and hasattr(lib, k.single) and hasattr(lib, k.multi)
    assert (hip_ops._KINDS["convk"].single, hip_ops._KINDS["convk"].multi) == ("savfi_convk_filters_f32", "savfi_convk_filters_multi_f32")
    for kind, form in (("wino", 0), ("wino2", 2)):
        k = hip_ops._KINDS[kind]
        assert (k.form, k.single, k.multi) == (form, "savfi_conv3x3_filters_form_f32", "savfi_conv3x3_filters_multi_form_f32")


def test_the_launches_cut_their_buffers_as_before(monkeypatch):
    """The real _make_filters / _filters_multi on host tensors, the C call left out: names, sizes and the slices of the one buffer."""
    names = []
    monkeypatch.setattr(_hip, "launch", lambda name, fn, **kw: names.append(name))
    monkeypatch.setattr(hip_ops, "_raw_stream", lambda: 0)
    monkeypatch.setattr(ref, "workspace_floats", hip_ops._workspace_floats)
    ws = [torch.zeros(s) for s in ((64, 64, 3, 3), (4, 32, 6, 3, 3), (51, 64, 3, 3), (2, 128, 64, 3, 3), (192, 192, 3, 3))]
    jobs = [(w, f, b) for w, (f, b) in zip(ws, [(True, True), (True, False), (False, True), (True, True), (True, True)])]
    for kind in TIMER:
        for js in (jobs, jobs + [(torch.zeros(64, 6, 5, 5), True, True)] if kind == "convk" else jobs[1:3]):
            names.clear()
            made = hip_ops._filters_multi(kind, js)
            assert names == [TIMER[kind] + "_multi"]
            cuts, total = ref.filters_multi_layout(kind, js)
            base = next(t for pair in made for t in pair if t is not None)
            assert base.storage_offset() == 0 and base.untyped_storage().nbytes() == 4 * total
            for (tf, tb), (of, nf, ob, nb), (w, f, b) in zip(made, cuts, js):
                for t, off, n, want in ((tf, of, nf, f), (tb, ob, nb, b)):
                    assert (t is not None) == bool(want) and n % 64 == 0
                    if want:
                        assert (t.storage_offset(), t.numel()) == (off, n) and t.untyped_storage().data_ptr() == base.untyped_storage().data_ptr()
                names.clear()
                sf, sb = hip_ops._make_filters(kind, w, f, b)
                assert names == [TIMER[kind]]
                for t, n, want in ((sf, nf, f), (sb, nb, b)):
                    assert (t is not None) == bool(want) and (not want or (t.numel() + 63) // 64 * 64 == n)
    assert hip_ops._filters_multi("wino", []) == [] and not names[1:]
    for w, want in zip(ws, [(1, 64, 64, 3), (4, 32, 6, 3), (1, 51, 64, 3), (2, 128, 64, 3), (1, 192, 192, 3)]):
        assert hip_ops._filter_shape(w) == ref._filter_shape(w) == want


def test_report_the_host_time_of_module_cache_hits(sides):
    """Not a gate: the host time of 10^5 hits in a module's cache through the transcription and through hip_ops.filter_lookup."""
    w = torch.zeros(8, 8, 3, 3)
    took = {}
    for name, lookup in (("transcription", ref._filters), ("filter_lookup", hip_ops.filter_lookup)):
        cache = {}
        lookup("convk", w, True, True, cache)
        best = float("inf")
        for _ in range(3):
            t0 = time.perf_counter()
            for _ in range(100000):
                lookup("convk", w, True, True, cache)
            best = min(best, time.perf_counter() - t0)
        took[name] = best
    print("10^5 module-cache hits: transcription %.1f ms, filter_lookup %.1f ms" % (1e3 * took["transcription"], 1e3 * took["filter_lookup"]))
