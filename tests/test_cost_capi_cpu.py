"""The cost-minimising objective (CEM_VARIANT_COST), the parts that need no GPU: what the host-side C ABI accepts and refuses, that a cost
handle's workspace and tile plan are the safe variant's, and the NumPy restatement of the objective against hand-written arrays.
(tests/test_warm_capi_cpu.py::test_planning_kernels_keep_their_register_counts covers the device side: every planning kernel keeps
its registers with the new reduce kernel present, whose name it admits.)"""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from ethz_safe_learning_amd import _capi
from ethz_safe_learning_amd.planner import PlannerConfig, ScorerConfig, plan_tiles, to_c_config
from oracle import cem_oracle as o
from tests import cost_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cfg(**kw):
    base = dict(obs_dim=60, act_dim=2, ensemble_size=5, particles=5, n_samples=2000, horizon=30, n_elite=200, iterations=5,
                scorer=ScorerConfig(goal_slice=(3, 19), cost_kinds=[(22, 38, 0.2)]), act_low=[-1, -1], act_high=[1, 1])
    base.update(kw)
    return PlannerConfig(**base)


SHAPES = {'B2': dict(),
          'safe_cem_mpc': dict(ensemble_size=15, particles=45, n_samples=500, horizon=8, n_elite=20, iterations=9),
          'B4': dict(n_samples=20000, n_elite=2000),
          'wide_tanh': dict(units=256, activation='tanh', n_samples=150, horizon=8, n_elite=15),
          'bf16x3_ragged': dict(precision='bf16x3', ensemble_size=3, particles=3, n_samples=97 * 3, horizon=33, n_elite=7)}


@pytest.mark.parametrize('shape', list(SHAPES))
def test_cost_variant_takes_the_safe_variants_workspace_and_tiles(built_lib, shape):
    safe, cost = _cfg(variant='safe', **SHAPES[shape]), _cfg(variant='cost', **SHAPES[shape])
    cs, ck = to_c_config(safe), to_c_config(cost)
    assert (cs.variant, ck.variant) == (1, 2) == (_capi.CEM_VARIANT_SAFE, _capi.CEM_VARIANT_COST)
    ws = built_lib.cem_workspace_bytes(C.byref(cs))
    assert ws > 0 and built_lib.cem_workspace_bytes(C.byref(ck)) == ws
    (rc_s, tiles_s), (rc_k, tiles_k) = plan_tiles(safe), plan_tiles(cost)
    assert rc_s == rc_k and len(tiles_s) > 0
    np.testing.assert_array_equal(tiles_s, tiles_k)
    if shape in ('B2', 'safe_cem_mpc'):                                  # what batch handles serve
        assert built_lib.cem_batch_workspace_bytes(C.byref(ck), 4) == built_lib.cem_batch_workspace_bytes(C.byref(cs), 4) > 0


def test_header_and_binding_name_the_variant(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'cem_mpc.h')).read()
    assert re.search(r'CEM_VARIANT_CEM = 0 [^,]*, CEM_VARIANT_SAFE = 1 [^,]*, CEM_VARIANT_COST = 2', hdr)
    assert '#define CEM_ABI_VERSION 4' in hdr and built_lib.cem_abi_version() == 4
    with pytest.raises(ValueError):
        to_c_config(_cfg(variant='costs'))


def test_unknown_variant_is_an_invalid_argument(built_lib):
    c = to_c_config(_cfg(variant='cost'))
    c.variant = 3
    assert built_lib.cem_workspace_bytes(C.byref(c)) == 0
    assert built_lib.cem_plan_tiles_host(C.byref(c), None, None, None, 0) == 1          # CEM_ERR_INVALID_ARG
    c.variant = -1
    assert built_lib.cem_plan_tiles_host(C.byref(c), None, None, None, 0) == 1


def test_cost_variant_is_one_rank_only(built_lib):
    c = to_c_config(_cfg(variant='cost', world_size=2, rank=1))
    assert built_lib.cem_plan_tiles_host(C.byref(c), None, None, None, 0) == 2          # CEM_ERR_UNSUPPORTED
    assert built_lib.cem_workspace_bytes(C.byref(c)) == 0
    c = to_c_config(_cfg(variant='safe', world_size=2, rank=1))
    assert built_lib.cem_plan_tiles_host(C.byref(c), None, None, None, 0) == 0          # the safe variant still shards


def test_restatement_against_hand_written_arrays():
    """2 particles x 3 candidates x 3 steps, every row at the goal from step 0: the cost objective counts every step's cost (the state
    after the last step is not scored, `<=` is inclusive), the done-masked safe objective would count none."""
    got = cc.mean_cost_scores(cc.HAND_TRAJ, 2, 3, cc.HAND_SP)
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, cc.HAND_SCORES)
    np.testing.assert_array_equal(got, np.array([-1.5, 0.0, -2.5], np.float32))
    bytes_ = cc.cost_bytes(cc.HAND_TRAJ, cc.HAND_SP)
    np.testing.assert_array_equal(bytes_, np.array([[1, 0, 1, 0, 0, 1], [1, 0, 0, 1, 0, 1], [0, 0, 1, 0, 0, 1]], np.float32))
    np.testing.assert_array_equal(cc.scores_from_bytes(bytes_.astype(np.uint8).reshape(3, 2, 3), 2, 3), cc.HAND_SCORES)
    # the done mask of safe_cem_mpc.py:89 would have zeroed all of it: every row reaches the goal at step 0
    _, reached = o.reward(cc.HAND_TRAJ[:, 0], cc.HAND_TRAJ[:, 1], cc.HAND_SP)
    assert reached.all()
    masked = o.compute_objective_safe(cc.HAND_TRAJ, 2, 3, cc.HAND_SP, 0.3)
    assert (masked > -50).all() and not np.array_equal(masked, got)
    # fp64 in, fp64 out, same values (quarters and halves are exact)
    np.testing.assert_array_equal(cc.mean_cost_scores(cc.HAND_TRAJ.astype(np.float64), 2, 3, cc.HAND_SP), cc.HAND_SCORES.astype(np.float64))


def test_restated_loop_runs_on_handed_in_scores():
    """plan_cost with the scores handed in: elites are the top-k with ties to the lowest index, best-so-far moves on strict > only."""
    rng = np.random.default_rng(3)
    N, H, A, I, k = 12, 3, 2, 3, 4
    cfg = o.PlanConfig(horizon=H, iterations=I, n_samples=N, n_elite=k, particles=2, ensemble_size=2)
    ea = rng.standard_normal((I, N, H, A)).astype(np.float32)
    seen = []

    def score_fn(it, actions):
        seen.append(actions.copy())
        return np.where(np.arange(N) % 3 == 0, np.float32(-0.0), np.float32(-0.5))      # candidates 0, 3, 6, 9 tie at the top
    a, s, it = cc.plan_cost(None, None, None, None, [-1, -1], [1, 1], ea, None, np.zeros(A, np.float32), cfg, None, score_fn=score_fn)
    assert it == I and s == 0.0
    np.testing.assert_array_equal(a, seen[0][0, 0])                                       # the first iteration's lowest tied index; later ties do not replace it
