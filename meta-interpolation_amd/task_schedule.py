"""What the three task modes (sequential loop, lockstep, hipGraph replays) decide the same way: when a target pass runs, which
rows of the meta-batch a group of tasks reads, whether a pass is differentiated."""
import contextlib

import torch


def target_schedule(num_steps, msl, training):
    """The target passes of one task, in order, as (s, index into the importance vector or None, with_grad): the pass runs on W_s,
    the weights after s updates, and its loss counts importance[index] times (None: once).  MAML++'s multi-step loss (`msl`, as
    forward() computes it: training only) has a pass after every step; otherwise there is one pass on W_S, which validation runs
    without autograd.

    num_step as the plugin sees it in a multi-step-loss pass on W_s: s - 1 from the eager loops, as in the reference, s from the
    graphs.  No plugin reads it; each mode keeps its value."""
    assert training or not msl, "the multi-step loss is a training loss"
    if not msl:
        return [(num_steps, None, training)]
    assert num_steps > 0, "the multi-step loss without an inner step has no target pass"
    return [(t + 1, t, True) for t in range(num_steps)]


def task_picker(frames, ids):
    """pick(i) -> frames[i] of the tasks `ids`: a slice where they are consecutive, index_select otherwise."""
    ids = list(ids)
    if ids == list(range(ids[0], ids[0] + len(ids))):
        return lambda i: frames[i][ids[0]:ids[0] + len(ids)]
    sel = torch.as_tensor(ids, device=frames[0].device)
    return lambda i: frames[i].index_select(0, sel)


def autograd_mode(with_grad):
    """The caller's autograd mode for a pass that is differentiated, no_grad for one that is not."""
    return contextlib.nullcontext() if with_grad else torch.no_grad()
