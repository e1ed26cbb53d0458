"""The lower-tail particle objective (cem_planner_set_particle_objective, CEM_PARTICLES_LOWER_TAIL), the parts that need no GPU: the two
symbols, what they refuse without a handle, risk_particles, config_key, the NumPy restatement against hand-written arrays and the new
kernel's code-object metadata.  (tests/test_warm_capi_cpu.py::test_planning_kernels_keep_their_register_counts covers the other
kernels: every one keeps its registers with the new kernel present, whose name it admits.)"""
import ctypes as C
import dataclasses
import os
import re

import numpy as np
import pytest

from ethz_safe_learning_amd import _capi, planner
from ethz_safe_learning_amd.planner import PlannerConfig, ScorerConfig, config_key, risk_particles, to_c_config
from oracle import cem_oracle as o
from tests import helpers as hp
from tests import risk_cases as rc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('cem_planner_set_particle_objective', 'cem_planner_get_particle_objective')


def _cfg(**kw):
    base = dict(obs_dim=60, act_dim=2, ensemble_size=5, particles=5, n_samples=2000, horizon=30, n_elite=200, iterations=5,
                scorer=ScorerConfig(goal_slice=(3, 19), cost_kinds=[(22, 38, 0.2)]), act_low=[-1, -1], act_high=[1, 1])
    base.update(kw)
    return PlannerConfig(**base)


def test_symbols_are_declared_exported_and_listed(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'cem_mpc.h')).read()
    for name in SYMBOLS:
        assert re.search(r'^int %s\(' % name, hdr, re.M), name
        assert name in _capi.EXPORTED_SYMBOLS
        assert getattr(built_lib, name) is not None
    assert re.search(r'CEM_PARTICLES_MEAN = 0, CEM_PARTICLES_LOWER_TAIL = 1', hdr)
    assert (_capi.CEM_PARTICLES_MEAN, _capi.CEM_PARTICLES_LOWER_TAIL) == (0, 1)
    assert planner.PARTICLE_OBJECTIVES == {'mean': 0, 'lower_tail': 1}


def test_null_handle_is_an_invalid_argument(built_lib):
    kind, m = C.c_int32(7), C.c_int32(7)
    for k, mm in ((0, 0), (1, 1), (2, 1)):
        assert built_lib.cem_planner_set_particle_objective(None, k, mm) == 1           # CEM_ERR_INVALID_ARG
    assert built_lib.cem_planner_get_particle_objective(None, C.byref(kind), C.byref(m)) == 1
    assert (kind.value, m.value) == (7, 7)                                                # nothing written


RISK_TABLE = [((0.2, 5), 1), ((0.1, 45), 5), ((0.07, 100), 7), ((1.0, 5), 5), ((1e-6, 5), 1),
              ((0.2, 45), 9), ((0.5, 5), 3), ((0.21, 5), 2), ((1.0, 1), 1), ((0.3, 10), 3), ((0.999, 45), 45), ((0.5, 128), 64)]


@pytest.mark.parametrize('args,want', RISK_TABLE)
def test_risk_particles_table(args, want):
    got = risk_particles(*args)
    assert got == want and isinstance(got, int)


@pytest.mark.parametrize('level', [0, 0.0, -0.1, -1, 1.0000001, 2, float('nan'), float('inf')])
def test_risk_particles_rejects_levels_outside_the_half_open_unit_interval(level):
    with pytest.raises(ValueError):
        risk_particles(level, 5)


def test_config_key_tells_the_settings_apart():
    keys = [config_key(_cfg(worst_particles=w)) for w in (0, 1, 2)]
    assert len(set(keys)) == 3
    assert config_key(_cfg()) == keys[0] and _cfg().worst_particles == 0
    # not a field of cem_config_t (its size is part of the ABI): the C configuration is the same bytes whatever the setting
    assert bytes(to_c_config(_cfg(worst_particles=2))) == bytes(to_c_config(_cfg()))


def test_restatement_against_hand_written_arrays():
    for m, want in rc.HAND_TAIL.items():
        got = rc.lower_tail_values(rc.HAND_RETURNS, m)
        assert got.dtype == np.float32
        np.testing.assert_array_equal(got, want, err_msg='m = %d' % m)
    # the issue's example: the mean cannot tell [9, 9, 9, 9, -40] from [-1] * 5 (about -1 both), the worst particle can
    mean = rc.HAND_RETURNS.sum(axis=0, dtype=np.float32) / np.float32(5)
    assert abs(mean[0] - mean[1]) < 0.25 and rc.HAND_TAIL[1][0] == -40 and rc.HAND_TAIL[1][1] == -1
    # m = P: every particle, added in ascending order
    np.testing.assert_array_equal(rc.lower_tail_values(rc.HAND_RETURNS, 5)[:2], np.array([np.float32(-4) / np.float32(5), -1], np.float32))
    # order matters in fp32: ascending order first adds the small ones
    r = np.array([[1e8], [1.0], [-1e8], [1.0]], np.float32)
    assert rc.lower_tail_values(r, 4)[0] == np.float32(((np.float32(-1e8) + np.float32(1)) + np.float32(1)) + np.float32(1e8)) / np.float32(4)
    assert rc.tail_ms(1) == [1] and rc.tail_ms(2) == [1, 2] and rc.tail_ms(5) == [1, 2, 4, 5] and rc.tail_ms(45) == [1, 2, 44, 45]


def test_restated_safe_rows_are_pushed_by_100():
    alpha, beta = o.beta_prior()
    assert abs(float(alpha) - 1.2147) < 1e-3 and alpha == beta
    for thr, want in rc.HAND_UNSAFE.items():
        np.testing.assert_array_equal(rc.unsafe_flags(rc.HAND_COSTS, 5, thr), want, err_msg=str(thr))
    got = rc.scores(rc.HAND_RETURNS, 1, rc.HAND_COSTS, 0.5)
    np.testing.assert_array_equal(got, np.array([-40., -101., -3., -7.], np.float32))
    got = rc.scores(rc.HAND_RETURNS, 2, rc.HAND_COSTS, 0.3)
    np.testing.assert_array_equal(got, np.array([-15.5, -101., -3., -103.5], np.float32))
    np.testing.assert_array_equal(rc.scores(rc.HAND_RETURNS, 2), rc.HAND_TAIL[2])
    np.testing.assert_array_equal(rc.top_k(np.array([1, 3, 3, 0, 3], np.float32), 2), [1, 2])      # ties to the lowest index


def test_shape_table_is_well_formed():
    for name, (P, N, H, E, thr) in rc.SHAPES.items():
        assert (P * N) % E == 0 and 0 < thr < 1, name
    assert {s[0] for s in rc.SHAPES.values()} == {1, 5, 16, 17, 45, 65, 128}
    assert {s[1] for s in rc.SHAPES.values()} == {70, 130} and {s[2] for s in rc.SHAPES.values()} == {3, 8, 17, 33}


@pytest.fixture(scope='module')
def isa():
    return hp.device_assembly()


def test_tail_kernel_has_no_spills_and_no_scratch(isa):
    meta = hp.kernel_meta(isa, r'cem_constraint_tail_kernel')
    assert len(meta) == 1, list(meta)
    (name, d), = meta.items()
    assert hp.kernel_function_name(name) in hp.KERNELS_SINCE_WARM_START  # what test_planning_kernels_keep_their_register_counts admits
    assert d['vgpr_spill_count'] == 0 and d['private_segment_fixed_size'] == 0, d
    assert 0 < d['vgpr_count'] <= 64, d                                # 1024-thread blocks: two resident per CU need <= 64


def test_policies_take_a_risk_level_and_default_to_none():
    import inspect
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    assert inspect.signature(CemMpc.__init__).parameters['risk_level'].default is None
    assert dataclasses.fields(PlannerConfig)[-1].name == 'worst_particles'
