"""Where a fused convolution got its packed / transformed filters from before hip_ops.filter_lookup: the functions of hip_ops.py as they
stood at commit 5723b9f (_filters, filters_after_update, refresh_module_filters, the registry of constant weights, _prepacked_filters,
_note_filter_use, conv3x3_filters, convk_filters and the job bookkeeping of _filters_multi), transcribed line for line.

What touched the process is injected, so the transcription runs on host tensors: the two launches (`launch_single(timer name, kind,
weight, fwd, bwd)` for the body of a public function's make(), `launch_multi(kind, jobs)` for _filters_multi), the device test
(`is_cuda`, which also stands for _hip.require_cuda), the capture query (`capturing`) and the stream query (`current_stream`).  The lines
that count an event into EVENTS are additions; they change nothing.  tests/test_filter_store_cpu.py holds hip_ops to this file."""
import collections
import threading

PARENT_COMMIT = "5723b9fcc72e7303b6082ba47bef9bfba3b6af06"

# injected by the test
is_cuda = capturing = current_stream = launch_single = launch_multi = workspace_floats = None
EVENTS = collections.Counter()

_FILTER_CACHE_PER_MODULE = 6


def _filters(kind, weight, fwd, bwd, cache):
    make = convk_filters if kind == 'convk' else (conv3x3_filters if kind == 'wino' else (lambda w_, f_, b_: conv3x3_filters(w_, f_, b_, f2=True)))
    if cache is None or capturing():
        EVENTS['lookup_while_capturing'] += bool(capturing())
        return make(weight, fwd, bwd)
    key = (kind, weight.data_ptr(), weight._version, tuple(weight.shape), weight.device.index, current_stream())
    hit = cache.get(key)
    if hit is not None and (hit[0] is not None or not fwd) and (hit[1] is not None or not bwd):
        EVENTS['module_hit'] += 1
        return (hit[0] if fwd else None), (hit[1] if bwd else None)
    EVENTS['module_remake_for_direction'] += hit is not None
    pf, pb = make(weight, fwd or (hit is not None and hit[0] is not None), bwd or (hit is not None and hit[1] is not None))
    cache.pop(key, None)
    while len(cache) >= _FILTER_CACHE_PER_MODULE:
        EVENTS['module_eviction'] += 1
        cache.pop(next(iter(cache)))
    cache[key] = (pf, pb)
    return (pf if fwd else None), (pb if bwd else None)


PREPACK = True
_pack_plans = {}        # tuple of the update's weight shapes -> {index: [kind, fwd, bwd]}
_last_update = None     # (signature, {data_ptr: index}, outputs) of the newest update
_prepacked = {}         # (kind, data_ptr) -> (weight, version, filters_fwd, filters_bwd)


def _filter_shape(weight):
    T, Co, Ci = (1,) + tuple(weight.shape[:2]) if weight.dim() == 4 else tuple(weight.shape[:3])
    return int(T), int(Co), int(Ci), int(weight.shape[-1])


def filters_after_update(outs):
    global _last_update
    _prepacked.clear()
    if not PREPACK or not outs or not is_cuda(outs[0]):
        EVENTS['update_with_prepack_off'] += not PREPACK
        _last_update = None
        return
    sig = tuple(tuple(o.shape) for o in outs)
    _last_update = (sig, {o.data_ptr(): i for i, o in enumerate(outs)}, outs)
    plan = _pack_plans.get(sig)
    if not plan:
        return
    for kind in ('convk', 'wino', 'wino2'):
        jobs = [(outs[i], e[1], e[2]) for i, e in sorted(plan.items()) if e[0] == kind]
        for (w, _, _), (tf, tb) in zip(jobs, _filters_multi(kind, jobs)):
            _prepacked[(kind, w.data_ptr())] = (w, w._version, tf, tb)


def _filters_multi(kind, jobs):
    if not jobs:
        return []
    return launch_multi(kind, jobs)


def filters_multi_layout(kind, jobs):
    """The job bookkeeping of _filters_multi: ([(offset_fwd, floats_fwd, offset_bwd, floats_bwd)], floats of the one buffer)."""
    sizes, total = [], 0
    for w, f, b in jobs:
        T, Co, Ci, K = _filter_shape(w)
        if kind == 'convk':
            nf = workspace_floats("savfi_convk_filter_floats", T, Ci, Co, K, 0) if f else 0
            nb = workspace_floats("savfi_convk_filter_floats", T, Ci, Co, K, 1) if b else 0
        else:
            fbit = 2 if kind == 'wino2' else 0
            nf = workspace_floats("savfi_conv3x3_filter_floats", T, Ci, Co, 0 | fbit) if f else 0
            nb = workspace_floats("savfi_conv3x3_filter_floats", T, Ci, Co, 1 | fbit) if b else 0
        nf, nb = (nf + 63) // 64 * 64, (nb + 63) // 64 * 64          # 256-byte aligned slices
        sizes.append((total, nf, total + nf, nb))
        total += nf + nb
    return sizes, total


def refresh_module_filters(modules):
    if not PREPACK or capturing():
        return
    st = current_stream()
    jobs = {'convk': [], 'wino': [], 'wino2': []}
    for m in modules:
        cache, w = getattr(m, '_filters', None), getattr(m, 'weight', None)
        if not cache or w is None or not is_cuda(w) or not w.is_contiguous():
            continue
        for key in reversed(list(cache)):
            kind, ptr, ver, shape, dev, stream = key
            if ptr == w.data_ptr() and shape == tuple(w.shape) and stream == st:
                if ver != w._version:
                    old = cache[key]
                    jobs[kind].append((m, key, (w.detach(), old[0] is not None, old[1] is not None)))
                break
    for kind, items in jobs.items():
        EVENTS['refresh_launched'] += bool(items)
        for (m, key, (w, _, _)), made in zip(items, _filters_multi(kind, [it[2] for it in items])):
            m._filters.pop(key, None)
            m._filters[(kind, w.data_ptr(), w._version, tuple(w.shape), w.device.index, st)] = made


_const_weights = {}
_const_weights_lock = threading.Lock()      # --task_streams: the per-task Python threads register / evict concurrently


_CONST_WEIGHTS_MAX = 64         # a model that goes away without unregistering leaves its entries behind: oldest out (16 per SepConv net and stream)


def register_const_weight(w):
    with _const_weights_lock:
        while len(_const_weights) >= _CONST_WEIGHTS_MAX:
            _const_weights.pop(next(iter(_const_weights)), None)
        _const_weights[w.data_ptr()] = [w, w._version, {}]
    return w


def unregister_const_weight(w):
    with _const_weights_lock:
        _const_weights.pop(w.data_ptr(), None)


def _const_filters(kind, weight, fwd, bwd, make):
    e = _const_weights.get(weight.data_ptr()) if _const_weights else None
    if e is None or e[1] != weight._version or e[0].shape != weight.shape or capturing():
        return None
    have = e[2].setdefault((kind, current_stream()), [None, None])
    need_f, need_b = fwd and have[0] is None, bwd and have[1] is None
    EVENTS['const_make' if need_f or need_b else 'const_hit'] += 1
    if need_f or need_b:
        pf, pb = make(need_f, need_b)
        if need_f:
            have[0] = pf
        if need_b:
            have[1] = pb
    return (have[0] if fwd else None), (have[1] if bwd else None)


def _prepacked_filters(kind, weight, fwd, bwd):
    hit = _prepacked.get((kind, weight.data_ptr())) if _prepacked else None
    EVENTS['prepacked_miss_by_version'] += hit is not None and hit[1] != weight._version
    if hit is None or hit[1] != weight._version or hit[0].shape != weight.shape or (fwd and hit[2] is None) or (bwd and hit[3] is None):
        return None
    EVENTS['prepacked_hit'] += 1
    return (hit[2] if fwd else None), (hit[3] if bwd else None)


def _note_filter_use(kind, weight, fwd, bwd):
    if _last_update is None:
        return
    sig, index, _ = _last_update
    i = index.get(weight.data_ptr())
    if i is None or tuple(weight.shape) != sig[i]:
        return
    entry = _pack_plans.setdefault(sig, {}).get(i)
    if entry is None:
        EVENTS['plan_learned'] += 1
        _pack_plans[sig][i] = [kind, bool(fwd), bool(bwd)]
    elif entry[0] == kind:
        entry[1], entry[2] = entry[1] or bool(fwd), entry[2] or bool(bwd)
    else:
        EVENTS['plan_refused_for_another_kind'] += 1


def conv3x3_filters(weight, fwd=True, bwd=True, f2=False):
    kind, fbit = ('wino2', 2) if f2 else ('wino', 0)
    weight = weight.contiguous()
    assert is_cuda(weight)
    T, Co, Ci = (1,) + tuple(weight.shape[:2]) if weight.dim() == 4 else tuple(weight.shape[:3])
    assert tuple(weight.shape[-2:]) == (3, 3) and (fwd or bwd), weight.shape
    ready = _prepacked_filters(kind, weight, fwd, bwd)
    if ready is not None:
        return ready

    def make(fwd, bwd):
        return launch_single("conv3x3_filters", kind, weight, fwd, bwd)
    ready = _const_filters(kind, weight, fwd, bwd, make)
    if ready is not None:
        return ready
    _note_filter_use(kind, weight, fwd, bwd)
    return make(fwd, bwd)


def convk_filters(weight, fwd=True, bwd=True):
    weight = weight.contiguous()
    assert is_cuda(weight)
    T, Co, Ci = (1,) + tuple(weight.shape[:2]) if weight.dim() == 4 else tuple(weight.shape[:3])
    K = int(weight.shape[-1])
    assert weight.shape[-2] == K and (fwd or bwd), weight.shape
    ready = _prepacked_filters('convk', weight, fwd, bwd)
    if ready is not None:
        return ready

    def make(fwd, bwd):
        return launch_single("convk_filters", 'convk', weight, fwd, bwd)
    ready = _const_filters('convk', weight, fwd, bwd, make)
    if ready is not None:
        return ready
    _note_filter_use('convk', weight, fwd, bwd)
    return make(fwd, bwd)
