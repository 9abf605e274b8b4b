"""The one pass schedule of a task (meta_learning_system.target_schedule) and what the task modes make of it: the list itself,
the 's' / 't' order handed to MetaDAIN.replay_running_stats, and the plugin forwards the sequential and the lockstep loop issue."""
import pytest
import torch

from meta_interpolation_amd import synthetic
from tests.helpers import build_toy_system

T, F = True, False

# (num_steps, msl, training) -> [(updates the weights have had, index into the importance vector or None, with autograd)]
SCHEDULE = {
    (0, F, F): [(0, None, F)],
    (0, F, T): [(0, None, T)],
    (1, F, F): [(1, None, F)],
    (1, F, T): [(1, None, T)],
    (2, F, F): [(2, None, F)],
    (2, F, T): [(2, None, T)],
    (3, F, F): [(3, None, F)],
    (3, F, T): [(3, None, T)],
    (1, T, T): [(1, 0, T)],
    (2, T, T): [(1, 0, T), (2, 1, T)],
    (3, T, T): [(1, 0, T), (2, 1, T), (3, 2, T)],
}
FRONT_PASSES = {
    (0, F): 't', (1, F): 's t', (2, F): 's s t', (3, F): 's s s t',
    (1, T): 's t', (2, T): 's t s t', (3, T): 's t s t s t',
}


def test_target_schedule_equals_the_lists_written_out_here():
    from meta_interpolation_amd.meta_learning_system import target_schedule
    for (S, msl, training), want in SCHEDULE.items():
        assert target_schedule(S, msl, training) == want, (S, msl, training)
    for S in range(4):
        with pytest.raises(AssertionError):         # msl, as forward() computes it, implies training
            target_schedule(S, True, False)
    with pytest.raises(AssertionError):             # the multi-step loss without an inner step has no target pass
        target_schedule(0, True, True)


@pytest.mark.parametrize("attenuate", [False, True])
def test_front_passes_follow_the_schedule(attenuate):
    system = build_toy_system(batch=1)
    system.args.attenuate = attenuate
    lead = ['s'] if attenuate else []                # L2F: the embedding pass
    for (S, msl), want in FRONT_PASSES.items():
        for training in ((T,) if msl else (F, T)):
            assert system._front_passes(S, msl, training) == lead + want.split(), (S, msl, training)


# (batch, num_step, backup_running_statistics, grad enabled) of every plugin forward; toy system, 3 tasks, 2 steps, unfused pairs
PROBE = (1, 0, F, T)
SUPPORT = [(1, 0, T, T), (1, 0, T, T), (1, 1, F, T), (1, 1, F, T)]
SEQ_VAL = 3 * (SUPPORT + [(1, 2, F, F)])
LOCK_VAL = [(6, 0, T, T), (6, 1, F, T), (3, 2, F, F)]
TRACES = {
    # (task_batch, msl): (train, validation)
    (0, F): (3 * (SUPPORT + [(1, 2, F, T)]), SEQ_VAL),
    (0, T): (3 * [(1, 0, T, T), (1, 0, T, T), (1, 0, F, T), (1, 1, F, T), (1, 1, F, T), (1, 1, F, T)], SEQ_VAL),
    (3, F): ([PROBE, (6, 0, T, T), (6, 1, F, T), (3, 2, F, T)], LOCK_VAL),
    (3, T): ([PROBE, (6, 0, T, T), (3, 0, F, T), (6, 1, F, T), (3, 1, F, T)], LOCK_VAL),
}


@pytest.mark.parametrize("task_batch,msl", sorted(TRACES))
def test_forward_calls_of_the_sequential_and_the_lockstep_loop(task_batch, msl):
    system = build_toy_system(batch=3, steps=2, msl=msl, task_batch=task_batch)
    frames = synthetic.septuplet_batch(3, 16, 24)
    trace, forward = [], system.net.forward

    def recording(f0, f1, params=None, backup_running_statistics=False, num_step=0, **kw):
        trace.append((f0.shape[0], num_step, bool(backup_running_statistics), torch.is_grad_enabled()))
        return forward(f0, f1, params=params, backup_running_statistics=backup_running_statistics, num_step=num_step, **kw)
    system.net.forward = recording
    system.optimizer.step = lambda *a, **k: None
    want_train, want_val = TRACES[(task_batch, msl)]
    system.run_train_iter(data_batch=frames, epoch=0)
    assert trace == want_train
    del trace[:]
    system.run_validation_iter(data_batch=frames)
    assert trace == want_val
