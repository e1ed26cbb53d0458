"""The task scorer (cem_planner_set_task, cem_task_score), the parts that need no GPU: the symbols and the struct, what
the calls refuse without a handle, the NumPy mirror planner.task_objective against a plain float64 evaluation of the contract, the
kernel's code-object metadata, the option rule and the policies' constructor default."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from ethz_safe_learning_amd import _capi
from ethz_safe_learning_amd.planner import PlannerConfig, QuadraticTask, ScorerConfig, config_key, task_objective, to_c_config
from tests import helpers as hp
from tests import task_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('cem_planner_set_task', 'cem_planner_task_trajectories', 'cem_task_score')
INVALID_ARG = 1
CONFIG_BYTES, LAYOUT_BYTES = 712, 136        # sizeof(cem_config_t), sizeof(cem_layout_t) of ABI 4 (LP64), as before the feature
# the largest |mirror - float64| / max(1, |float64|) over the returns of test_mirror_against_float64's cases, measured on the CPU
MIRROR_ERROR_MEASURED = 2.9e-7


def test_symbols_are_declared_exported_and_listed(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'cem_mpc.h')).read()
    for name in SYMBOLS:
        assert re.search(r'^int %s\(' % name, hdr, re.M), name
        assert name in _capi.EXPORTED_SYMBOLS
        assert getattr(built_lib, name) is not None
    assert re.search(r'enum cem_task_kind \{ CEM_TASK_SAFETY_GYM = 0, CEM_TASK_QUADRATIC = 1 \};', hdr)
    assert (_capi.CEM_TASK_SAFETY_GYM, _capi.CEM_TASK_QUADRATIC) == (0, 1)
    assert [f[0] for f in _capi.CemTask._fields_] == ['kind', 'q', 'g', 'c', 'goal_mask', 'lo', 'hi', 'rho', 'goal_radius', 'reward_goal', 'reward_clip']
    assert re.search(r'#define CEM_ABI_VERSION 4\b', hdr) and built_lib.cem_abi_version() == 4
    mk = open(os.path.join(hp.CSRC, 'Makefile')).read()
    assert mk.count('cem_task_score.hip') == 2                                    # a prerequisite and a source of the one link line


def test_null_handle_is_an_invalid_argument(built_lib):
    task = _capi.CemTask(kind=_capi.CEM_TASK_QUADRATIC)
    assert built_lib.cem_planner_set_task(None, C.byref(task)) == INVALID_ARG
    assert built_lib.cem_planner_set_task(None, None) == INVALID_ARG
    assert built_lib.cem_planner_task_trajectories(None, None) == INVALID_ARG
    assert built_lib.cem_task_score(None, None, None, 1, 1, None, None) == INVALID_ARG


def test_structs_keep_their_sizes_and_the_header_compiles_as_c(tmp_path):
    assert C.sizeof(_capi.CemConfig) == CONFIG_BYTES and C.sizeof(_capi.CemLayout) == LAYOUT_BYTES
    cc = os.environ.get('CC', 'cc')
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include "cem_mpc.h"\nint main(void) { printf("%zu %zu %zu", sizeof(cem_config_t), sizeof(cem_layout_t), '
                   'sizeof(cem_task_t)); return 0; }\n')
    exe = tmp_path / 'sz'
    try:
        subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)], check=True, capture_output=True)
    except (OSError, subprocess.CalledProcessError) as e:
        pytest.fail('the header must compile as plain C: %r' % (getattr(e, 'stderr', e),))
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [CONFIG_BYTES, LAYOUT_BYTES, C.sizeof(_capi.CemTask)]


def test_the_task_is_part_of_the_cache_key_and_not_of_the_c_config():
    kw = dict(obs_dim=12, act_dim=2, ensemble_size=5, particles=5, n_samples=64, horizon=5, n_elite=8, iterations=3,
              scorer=ScorerConfig(goal_slice=(3, 7)), act_low=[-1, -1], act_high=[1, 1], units=32)
    off, on = PlannerConfig(**kw), PlannerConfig(task=QuadraticTask(q=1.0), **kw)
    other = PlannerConfig(task=QuadraticTask(q=np.arange(12.0)), **kw)
    assert off.task is None
    assert len({config_key(off), config_key(on), config_key(other)}) == 3
    assert bytes(to_c_config(off)) == bytes(to_c_config(on))


def test_tables_broadcast_and_refuse_other_shapes():
    t = QuadraticTask(q=2.0, g=[1.0, 2.0, 3.0], rho=[0.5, 0.25])
    tb = t.tables(3, 2)
    assert all(tb[k].dtype == np.float32 and tb[k].shape == (3,) for k in ('q', 'g', 'c', 'goal_mask', 'lo', 'hi')) and tb['rho'].shape == (2,)
    assert (tb['q'] == 2.0).all() and (tb['lo'] == -np.inf).all() and (tb['hi'] == np.inf).all() and (tb['c'] == 0).all()
    with pytest.raises(ValueError):
        t.tables(4, 2)
    w = QuadraticTask.to_target([1.0, 0.0, -1.0], weights=[1.0, 0.0, 2.0], action_weights=0.1, goal_radius=0.2, reward_goal=5.0)
    tb = w.tables(3, 1)
    assert tb['q'].tolist() == [1.0, 0.0, 2.0] and tb['goal_mask'].tolist() == [1.0, 0.0, 1.0] and tb['g'].tolist() == [1.0, 0.0, -1.0]


def _cases():
    for (O, A, H, rows, P) in tc.SHAPES:
        for variant in ('cem', 'safe', 'cost'):
            for seed in range(3):
                for clip in (True, False):
                    task = tc.task_for(O, A, seed, clip)
                    tr, act = tc.random_case(O, A, H, rows, P, seed)
                    tc.clear_thresholds(tr, task)
                    names = tc.craft(tr, task, boundaries=False)          # goal reached at t = 0, at the last step, never
                    yield (O, variant, seed, clip), task, tr, act, variant, names


def test_mirror_against_float64():
    """planner.task_objective against the contract in float64 (task_cases.objective_f64) on random and crafted trajectories of the
    kernel tests' four shapes, three variants, three seeds, with and without a reward clip.  No comparison operand lies within 1e-4 of
    its threshold (asserted), so cost bytes and done steps are EQUAL.  The returns: the largest |mirror - float64| / max(1, |float64|)
    measured over these cases is 2.9e-7 (returns down to -1.1e3: sums of up to 30 steps of up to 100 feature terms in float32); the
    bar is twice that."""
    worst, seen = 0.0, set()
    for what, task, tr, act, variant, names in _cases():
        r64, c64, d64, margin = tc.objective_f64(tr, act, task, variant)
        r32, c32, d32 = task_objective(tr, act, task, variant, return_done=True)
        assert margin > tc.NEAR, (what, margin)
        assert r32.dtype == np.float32 and np.array_equal(d32, d64), what
        if variant == 'cem':
            assert c32 is None and c64 is None
        else:
            assert c32.dtype == np.uint8 and np.array_equal(c32, c64), what
        H = act.shape[1]
        if variant != 'cost' and names:                                        # the crafted rows are what they are named
            assert d64[names['goal_at_0']] == 0 and d64[names['goal_at_last_step']] == H - 1 and d64[names['goal_never']] == H, what
        seen.add((variant, bool((d64 < H).any()), bool((d64 == H).any()), c64 is not None and bool(c64.any())))
        worst = max(worst, float((np.abs(r32.astype(np.float64) - r64) / np.maximum(1.0, np.abs(r64))).max()))
    print('mirror against float64: largest relative distance %.3g' % worst)
    assert worst <= 2 * MIRROR_ERROR_MEASURED, worst
    # both outcomes of done and non-zero cost bytes occur on the safe variant; the cost variant never ends an episode
    assert ('safe', True, True, True) in seen and not any(v == 'cost' and d for v, d, _, _ in seen)


def test_mirror_crafted_thresholds():
    """What the contract says ON the thresholds, in the mirror (the kernel is held to the mirror bit for bit on the GPU): a feature on a
    bound is no violation, one ulp outside is; near holds at exactly R2 and not one ulp outside; a NaN feature violates nothing, is
    never near and, with the clip on, costs the step exactly -clip."""
    O, A, H, rows, P = tc.SHAPES[1]
    task = tc.task_for(O, A, 0, True)
    tr, act = tc.random_case(O, A, H, rows, P, 0)
    names = tc.craft(tr, task)
    ret, costs, first = task_objective(tr, act, task, 'safe', return_done=True)
    assert costs[:, names['on_bounds']].sum() == 0
    assert costs[0, names['ulp_below_lo']] == 1 and costs[0, names['ulp_above_hi']] == 1
    assert first[names['near_exactly']] == 0 and first[names['near_ulp_outside']] == H
    assert costs[:, names['nan_feature']].sum() == 0 and first[names['nan_feature']] == H and np.isfinite(ret[names['nan_feature']])
    # without a clip the NaN step is -inf and so is the return; with the state a NaN on a DONE row (cem order: the step counts 0) it is a NaN
    ret_nc, _ = task_objective(tr, act, tc.task_for(O, A, 0, False), 'safe')
    assert ret_nc[names['nan_feature']] == -np.inf
    tr[names['nan_feature'], 0, :2] = 0.1                                      # near at s_0: done from step 0 (safe) / 1 (cem) on
    ret_d, _ = task_objective(tr, act, tc.task_for(O, A, 0, False), 'cem')
    assert ret_d.view(np.uint32)[names['nan_feature']] == 0x7fc00000


@pytest.fixture(scope='module')
def task_isa():
    """The device ISA of csrc/cem_task_score.hip, the kernel's own translation unit (helpers.unit_assembly: without the compiler the
    test FAILS)."""
    return hp.unit_assembly('cem_task_score.hip')


def test_the_kernel_has_no_spills_no_scratch_no_lds_and_no_atomics(task_isa):
    meta = hp.kernel_meta(task_isa, r'.', keys=('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size',
                                                'group_segment_fixed_size'))
    assert sorted({hp.kernel_function_name(n) for n in meta}) == ['cem_task_score_kernel'], sorted(meta)      # the unit holds this one alone
    assert len(meta) == 4                                                         # one / two quads per lane x 16-byte / element loads
    for name, d in meta.items():
        print(name, d)
        assert d['vgpr_spill_count'] == 0 and d['sgpr_spill_count'] == 0 and d['private_segment_fixed_size'] == 0, (name, d)
        assert d['group_segment_fixed_size'] == 0, (name, d)                      # the tables sit in registers
        assert 0 < d['vgpr_count'] <= 128 and 0 < d['sgpr_count'] <= 100, (name, d)     # (128: two workgroups of 256 a SIMD's registers hold four times over)
        body = hp.kernel_bodies(task_isa, re.escape(name))[name]
        assert not any(re.match(r'(global|flat|buffer)_atomic', l) for l in body)
        assert not any(re.match(r'scratch_', l) for l in body)
        assert not any(re.match(r'v_(fma|fmac|mad|mac|pk_fma)_f32', l) for l in body), name      # products and sums are rounded separately
        wide = any(re.match(r'global_load_dwordx4', l) for l in body)
        assert wide, name                                                         # (the tables at least; the 16-byte path its states too)


def test_the_option_rule():
    """admit() (csrc/cem_plan_options.h) through the library's own handles needs a GPU; the rule's text is held here: one block, which
    names the four refusals."""
    src = open(os.path.join(hp.CSRC, 'cem_plan_options.h')).read()
    assert re.search(r'if \(o\.task != 0 && \(f\.W > 1 \|\| o\.comm \|\| f\.batch \|\| !f\.can_task\)\) return CEM_ERR_UNSUPPORTED;', src)
    assert src.count('o.task') == 1


def test_policy_constructor_default_is_off_and_generate_actions_refuses():
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    from ethz_safe_learning_amd.simba.policies.safe_cem_mpc import SafeCemMpc
    assert inspect.signature(CemMpc.__init__).parameters['task'].default is None
    assert 'kwargs' in inspect.signature(SafeCemMpc.__init__).parameters                  # ... which SafeCemMpc passes through
    pol = CemMpc.__new__(CemMpc)
    pol.task = QuadraticTask(q=1.0)
    with pytest.raises(ValueError, match='batch handle'):
        pol.generate_actions(np.zeros((2, 3), np.float32))


def test_the_closed_loop_reference_figures_are_the_references():
    """The bars of tests/test_gpu_task_scorer.py's double integrator, measured here: the NumPy CEM of task_cases.reference_closed_loop,
    seeds 0 .. 4, ends with a stage cost of at most 2.61e-4 and never moves faster than 0.911 (the box is 1.0)."""
    out = [tc.reference_closed_loop(s) for s in range(5)]
    print('closed-loop reference:', out)
    assert max(c for c, _ in out) <= tc.REFERENCE_WORST_STAGE_COST and max(c for c, _ in out) > 0.9 * tc.REFERENCE_WORST_STAGE_COST
    assert max(v for _, v in out) <= tc.REFERENCE_WORST_SPEED < tc.VEL_BOX
