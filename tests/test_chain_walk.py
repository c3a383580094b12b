"""Host: eo_diffusion_amd/diffusion/chain.py -- the walk every sampler runs its step and jump bodies through, with recording fakes,
against the hand-written tables of tests/repaint_ref.py (the ones tests/test_gpu_repaint_resample.py pins the Philox keys of the
real samplers to)."""
import os
import subprocess
import sys

import pytest

from eo_diffusion_amd.diffusion import chain
from eo_diffusion_amd.diffusion.util import resample_plan
from tests.repaint_ref import EVALS, MOVES


def _record(T, resample):
    """(evaluations as (level, step stream), moves as {evaluation number: (a, b, (step, stream))}, jump ordinals, states seen)"""
    evals, moves, ordinals, states = [], {}, [], []

    def step(x, k, level, visit):
        assert k == len(evals)
        evals.append((level, chain.step_stream(visit)))
        states.append(x)
        return x + 1

    def jump(x, j, a, b, visits_of_b):
        moves[len(evals)] = (a, b, (b, chain.jump_stream(visits_of_b)))
        ordinals.append(j)
        states.append(x)
        return x + 100

    visits, jump_after = resample_plan("test", resample, T)
    out = chain.walk(0, visits, jump_after, step, jump)
    return evals, moves, ordinals, states, out


def test_resampled_walk_equals_the_hand_written_tables():
    evals, moves, ordinals, states, out = _record(8, (2, 2))
    assert evals == EVALS and moves == MOVES and ordinals == [0, 1, 2]
    assert out == 14 + 300                                            # every body's return value is the next body's state
    assert states[:5] == [0, 1, 2, 3, 103]                            # ... in order: three steps, the jump after the third, a step
    assert chain.X_T_STREAM == 0 and (8, chain.X_T_STREAM) not in set(evals) | {key for _, _, key in moves.values()}


def test_plain_descent_is_stream_1_throughout():
    evals, moves, ordinals, states, out = _record(8, None)
    assert evals == [(i, 1) for i in range(7, -1, -1)] and moves == {} and ordinals == [] and out == 8


def test_walk_with_a_progress_bar_is_the_same_walk():
    evals = []
    visits, jump_after = resample_plan("test", (2, 2), 8)
    chain.walk(None, visits, jump_after, lambda x, k, level, visit: evals.append((level, chain.step_stream(visit))),
               lambda x, j, a, b, n: None, desc="test")
    assert evals == EVALS


def test_pick_takes_a_sequence_or_a_callable():
    assert chain.pick([5, 6, 7], 1) == 6 and chain.pick(lambda k: 10 * k, 3) == 30
    with pytest.raises(IndexError):
        chain.pick([5], 1)


def test_the_module_is_host_only():
    code = ("import sys, eo_diffusion_amd.diffusion.chain; "
            "assert 'torch' not in sys.modules and 'eo_diffusion_amd._lib' not in sys.modules, sorted(m for m in sys.modules if 'eo_' in m)")
    subprocess.run([sys.executable, "-c", code], check=True, cwd=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
