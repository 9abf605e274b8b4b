"""The routing predicates of the fused convolutions as they stood before hip_ops.conv_route, transcribed over integers: shapes are tuples,
the knobs a dict `k` (DEFAULTS: the shipped values), the F(4x4) workgroup count tests.conv_ref.f4_plan (tied to the library by
test_conv_plan_cpu.py).  `route` is what the two autograd functions then did with them, forward and backward.  tests/test_conv_route_cpu.py
holds hip_ops to this file."""
from tests.conv_ref import f4_plan

DEFAULTS = dict(
    WINOGRAD_CONV=True, WINO_MIN_TILES_FWD=700, WINO_MIN_TILES_BWD=700, WINO_MIN_TILES_FWD_BATCHED=100, WINO_MIN_TILES_BWD_BATCHED=100,
    WGRAD_MIN_PIXELS=3000, WGRAD_MIN_CI=16, WGRAD_WINO=True, WGRAD_WINO_MIN_GFLOP=5.0, WGRAD_WINO_MIN_PIXELS=192,
    CONVK=True, CONVK_3X3_MIN_PIXELS=700, CONVK_WGRAD3_RING_MIN_PIXELS=3000, CONVK_WGRAD3_RING_SMALL_MIN_PIXELS=64, CONVK_WGRAD3=True,
    CONVK_WGRAD3_RING=True, WINO4_MIN_WORKGROUPS=180, WINO4_MIN_PIXELS=400, TASKS_MIN_TILES_FWD=1, TASKS_MIN_TILES_BWD=1,
    TASKS_WGRAD_MIN_PIXELS=3000)


def _one(v, k):
    return (v == k) if isinstance(v, int) else all(t == k for t in v)


def _pad(padding):
    return padding if isinstance(padding, int) else (padding[0] if padding[0] == padding[1] else -1)


def wino4_workgroups(N, Ci, Co, H, W, pad, mode=0):
    plan = f4_plan(N, Ci, Co, H, W, pad, mode)
    return plan["workgroups"] if plan else 0


def wgrad_wino(k, N, Ci, Co, Ho, Wo):
    if Ci * (Ho + 2) * (Wo + 2) >= (1 << 28) or Co * Ho * Wo >= (1 << 28):
        return False
    return bool(k["WGRAD_WINO"] and Ho * Wo >= k["WGRAD_WINO_MIN_PIXELS"] and 18e-9 * Ci * Co * Ho * Wo * N >= k["WGRAD_WINO_MIN_GFLOP"])


def convk_wgrad_preferred(k, K, Ci, Co, Ho, Wo, direct=False, N=None):
    if not k["CONVK"] or K not in (3, 5, 7):
        return False
    if K != 3 or direct:
        return True
    if not k["CONVK_WGRAD3"]:
        return False
    if Ci >= 48 and Co >= 48 and Ho * Wo >= k["CONVK_WGRAD3_RING_MIN_PIXELS"] and k["CONVK_WGRAD3_RING"]:
        return True
    if N is not None and Ci >= 48 and Co >= 48 and Ho * Wo >= k["CONVK_WGRAD3_RING_SMALL_MIN_PIXELS"] and k["CONVK_WGRAD3_RING"] \
            and not wgrad_wino(k, N, Ci, Co, Ho, Wo):
        return True
    return (Ci <= 32 and Ho * Wo >= 16384) or (Co >= 192 and Ho * Wo >= 4096)


def convk_geometry(w, stride, padding, dilation, groups):
    K = w[-1]
    if K not in (3, 5, 7) or w[-2] != K or not _one(stride, 1) or not _one(dilation, 1) or groups != 1:
        return None
    pad = _pad(padding)
    if pad < 0 or pad > K - 1:
        return None
    return K, pad


def convk_eligible(k, x, w, stride, padding, dilation, groups=1, direct=False):
    if not k["CONVK"] or len(x) != 4:
        return False
    geo = convk_geometry(w, stride, padding, dilation, groups)
    if geo is None:
        return False
    K, pad = geo
    H, W = x[2:]
    Ho, Wo = H + 2 * pad - K + 1, W + 2 * pad - K + 1
    Co, Ci = w[-4], w[-3]
    if Ho < 1 or Wo < 1 or Ci * H * W >= (1 << 29) or Co * Ho * Wo >= (1 << 29):
        return False
    if K != 3 or direct:
        return True
    if not (Ho * Wo >= k["CONVK_3X3_MIN_PIXELS"] and (Ci <= 8 or (Ci >= 64 and Co >= 64 and Co % 64 == 0))):
        return False
    return Ci <= 8 or pad > 1 or not k["WINOGRAD_CONV"] or wino4_workgroups(x[0], Ci, Co, H, W, pad) < k["WINO4_MIN_WORKGROUPS"]


def wino_form2(k, x, w, pad):
    n = wino4_workgroups(x[0], w[-3], w[-4], x[2], x[3], pad)
    if n <= 0:
        return False
    return n < k["WINO4_MIN_WORKGROUPS"] or (x[2] + 2 * pad - 2) * (x[3] + 2 * pad - 2) < k["WINO4_MIN_PIXELS"]


def conv3x3_eligible(k, x, w, stride, padding, dilation, groups, backward=False):
    if not k["WINOGRAD_CONV"] or len(x) != 4:
        return False
    pad = _pad(padding)
    if tuple(w[2:]) != (3, 3) or not _one(stride, 1) or not _one(dilation, 1) or groups != 1 or pad not in (0, 1):
        return False
    N, _, H, W = x
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    if Ho < 1 or Wo < 1 or H * W < 4:
        return False
    tiles = N * ((Ho + 1) // 2) * ((Wo + 1) // 2)
    if N >= 2 and tiles >= (k["WINO_MIN_TILES_BWD_BATCHED"] if backward else k["WINO_MIN_TILES_FWD_BATCHED"]):
        return True
    return tiles >= (k["WINO_MIN_TILES_BWD"] if backward else k["WINO_MIN_TILES_FWD"])


def conv3x3_wgrad_eligible(k, x, w, stride, padding, dilation, groups):
    if not k["WINOGRAD_CONV"] or len(x) != 4:
        return False
    pad = _pad(padding)
    if tuple(w[2:]) != (3, 3) or not _one(stride, 1) or not _one(dilation, 1) or groups != 1 or pad not in (0, 1):
        return False
    _, Ci, H, W = x
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    fill = Wo / (64.0 * ((Wo + 63) // 64)) if Wo > 0 else 0.0
    if Ho > 0 and Wo > 0 and wgrad_wino(k, x[0], Ci, w[0], Ho, Wo):
        return True
    return Ci >= k["WGRAD_MIN_CI"] and Ho * Wo >= k["WGRAD_MIN_PIXELS"] and fill >= 0.85


def _is3x3s1(w, stride, padding, dilation):
    return tuple(w[-2:]) == (3, 3) and _one(stride, 1) and _one(dilation, 1) and _pad(padding) in (0, 1)


def conv3x3_tasks_eligible(k, x, w, stride, padding, dilation, backward=False):
    if not (k["WINOGRAD_CONV"] and len(x) == 4 and _is3x3s1(w, stride, padding, dilation)):
        return False
    pad = padding if isinstance(padding, int) else padding[0]
    N, _, H, W = x
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    if Ho < 1 or Wo < 1 or H * W < 4:
        return False
    return N * ((Ho + 1) // 2) * ((Wo + 1) // 2) >= (k["TASKS_MIN_TILES_BWD"] if backward else k["TASKS_MIN_TILES_FWD"])


def conv3x3_wgrad_tasks_eligible(k, x, w, stride, padding, dilation):
    if not (k["WINOGRAD_CONV"] and len(x) == 4 and _is3x3s1(w, stride, padding, dilation)):
        return False
    pad = padding if isinstance(padding, int) else padding[0]
    N, Ci, H, W = x
    Ho, Wo = H + 2 * pad - 2, W + 2 * pad - 2
    return Ho * Wo >= k["TASKS_WGRAD_MIN_PIXELS"] or (Ho > 0 and Wo > 0 and wgrad_wino(k, N, Ci, w[1], Ho, Wo))


def convk_reflect_eligible(k, x, w, pad):
    if len(w) != 4 or len(x) != 4 or pad < 1 or w[-1] != 2 * pad + 1:
        return False
    if pad >= x[2] or pad >= x[3]:
        return False
    return convk_eligible(k, x, w, 1, pad, 1, 1, False)


def unit16_route(k, x, w, pad):
    """conv3x3_unit16_supported up to the library's own answer about the launch plan"""
    return len(w) == 5 and conv3x3_tasks_eligible(k, x, w, 1, pad, 1) and not convk_eligible(k, x, w, 1, pad, 1, 1, False) \
        and not wino_form2(k, x, w, pad)


def route(k, x, w, stride, padding, dilation, groups=1, direct=False, reflect=False):
    """(fwd, dgrad, wgrad) as _ConvBiasAct (4-D w) / _ConvBiasActTasks (5-D w) chose them in forward and backward."""
    tasks = len(w) == 5
    if tasks:
        wino = lambda backward: conv3x3_tasks_eligible(k, x, w, stride, padding, dilation, backward)
        wgrad3 = conv3x3_wgrad_tasks_eligible(k, x, w, stride, padding, dilation)
    else:
        wino = lambda backward: conv3x3_eligible(k, x, w, stride, padding, dilation, groups, backward)
        wgrad3 = conv3x3_wgrad_eligible(k, x, w, stride, padding, dilation, groups)
    if convk_eligible(k, x, w, stride, padding, dilation, groups, direct):
        fwd = "convk"
    elif wino(False):
        fwd = "wino2" if wino_form2(k, x, w, _pad(padding)) else "wino"
    else:
        fwd = "aten"
    if fwd == "convk":
        dgrad = "convk"
    elif wino(True):
        dgrad = fwd if fwd in ("wino", "wino2") else "conv3x3"        # conv3x3(gz, w, ...) / conv3x3_tasks(gz, w, ...): no filter from the forward
    else:
        dgrad = "aten"
    geo = convk_geometry(w, stride, padding, dilation, groups)
    K = w[-1]
    if reflect or (geo is not None and (fwd == "convk" or K == 3)
                   and convk_wgrad_preferred(k, K, w[-3], w[-4], x[2] + 2 * geo[1] - K + 1, x[3] + 2 * geo[1] - K + 1, direct, x[0])):
        wgrad = "convk"
    elif wgrad3:
        wgrad = "conv3x3"
    else:
        wgrad = "aten"
    return fwd, dgrad, wgrad
