"""Linear outputs on a task (cem_planner_set_task_outputs) without a GPU: the NumPy mirror of cem_task_outputs_kernel
against the contract in float64, what the contract says on its thresholds, the equalities with a task without outputs, TaskOutputs and
its constructors, the C surface, the kernel's recorded resources and the closed loops' reference figures."""
import ctypes as C
import dataclasses
import json
import os
import re
import subprocess

import numpy as np
import pytest

from ethz_safe_learning_amd import StateZones, TaskOutputs, _capi
from ethz_safe_learning_amd.planner import QuadraticTask, TrackingTask, output_terms, task_objective, tracking_objective
from tests import helpers as hp
from tests import output_cases as oc
from tests import task_cases as tc
from tests import tracking_cases as tk
from tests import zone_cases as zc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID_ARG = 1
U, F = np.uint32, np.float32


def _objective(task, tr, act, variant, k0=0, prev=None, **kw):
    if isinstance(task, TrackingTask):
        return tracking_objective(tr, act, task, variant, k0=k0, prev_action=prev, **kw)
    return task_objective(tr, act, task, variant, **kw)


def _same(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
        else:
            np.testing.assert_array_equal(x.view(U) if x.dtype == F else x, y.view(U) if y.dtype == F else y)


# ---------------------------------------------------------------------------------------------------------------------------------
# the C surface and the build
# ---------------------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_listed(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'cem_mpc.h')).read()
    assert re.search(r'^int cem_planner_set_task_outputs\(', hdr, re.M)
    assert 'cem_planner_set_task_outputs' in _capi.EXPORTED_SYMBOLS and built_lib.cem_planner_set_task_outputs is not None
    assert re.search(r'#define CEM_TASK_MAX_OUTPUTS 16\b', hdr) and _capi.CEM_TASK_MAX_OUTPUTS == 16
    assert [f[0] for f in _capi.CemTaskOutputs._fields_] == ['n_outputs', 'matrix', 'weight', 'target', 'linear', 'near', 'lo', 'hi', 'terminal',
                                                              'ref_rows', 'reference']
    assert re.search(r'#define CEM_ABI_VERSION 4\b', hdr) and built_lib.cem_abi_version() == 4
    mk = open(os.path.join(hp.CSRC, 'Makefile')).read()
    assert mk.count('cem_task_outputs.hip') == 2                                  # a prerequisite and a source of the one link line
    assert built_lib.cem_planner_set_task_outputs(None, None) == INVALID_ARG
    assert built_lib.cem_planner_set_task_outputs(None, C.byref(_capi.CemTaskOutputs(n_outputs=1))) == INVALID_ARG
    # one new fact and one new line in admit(); the kernel is a kind of the one tile behind a wrapper of one line
    opts = open(os.path.join(hp.CSRC, 'cem_plan_options.h')).read()
    assert 'can_outputs' in opts and re.search(r'if \(o\.outputs != 0 && !f\.can_outputs\) return CEM_ERR_UNSUPPORTED;', opts)
    src = open(os.path.join(hp.CSRC, 'cem_task_outputs.h')).read()
    code = src[src.index('#pragma once'):]
    assert re.search(r'void cem_task_outputs_kernel\(const TaskParams p\) \{ cem_task_rows<NT, VEC, CEM_TASK_KIND_OUTPUTS>\(p\); \}', code)
    assert '__shfl' not in code and 'ballot' not in code and 'struct ' not in code


def test_the_struct_compiles_as_c_and_the_tasks_keep_their_sizes(tmp_path):
    cc = os.environ.get('CC', 'cc')
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include "cem_mpc.h"\nint main(void) { cem_task_outputs_t o = {0}; printf("%zu %zu %zu %zu %d %d", '
                   'sizeof(cem_task_t), sizeof(cem_task_tracking_t), sizeof(cem_task_zones_t), sizeof o, o.n_outputs, CEM_TASK_MAX_OUTPUTS); return 0; }\n')
    exe = tmp_path / 'sz'
    try:
        subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)], check=True, capture_output=True)
    except (OSError, subprocess.CalledProcessError) as e:
        pytest.fail('the header must compile as plain C: %r' % (getattr(e, 'stderr', e),))
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [C.sizeof(_capi.CemTask), C.sizeof(_capi.CemTaskTracking), C.sizeof(_capi.CemTaskZones), C.sizeof(_capi.CemTaskOutputs), 0, 16]
    assert got[:3] == [80, 32, 64]                                                # (as before outputs)


@pytest.fixture(scope='module')
def outputs_isa():
    """The device ISA of csrc/cem_task_outputs.hip, the kernel's own translation unit (helpers.unit_assembly: without the compiler the
    test FAILS)."""
    return hp.unit_assembly('cem_task_outputs.hip')


def test_the_kernel_has_no_spills_no_scratch_and_the_recorded_registers_and_lds(outputs_isa):
    meta = hp.kernel_meta(outputs_isa, r'.', keys=('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size',
                                                   'group_segment_fixed_size'))
    assert sorted({hp.kernel_function_name(n) for n in meta}) == ['cem_task_outputs_kernel'], sorted(meta)    # the unit holds this one alone
    assert len(meta) == 4                                                         # one / two quads per lane x 16-byte / element loads
    golden = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'task_outputs_resources.json')))
    assert sorted(golden) == sorted(meta)
    for name, d in meta.items():
        print(name, d)
        assert d['vgpr_spill_count'] == 0 and d['sgpr_spill_count'] == 0 and d['private_segment_fixed_size'] == 0, (name, d)
        assert {'vgpr_count': d['vgpr_count'], 'group_segment_fixed_size': d['group_segment_fixed_size']} == golden[name], (name, d, golden[name])
        assert d['group_segment_fixed_size'] == 16 * 128 * 4, (name, d)           # C, and nothing else
    # no fused multiply-add, no atomic and no scratch in the unit
    assert not re.search(r'\bv_(fma|fmac|mad|mac)_f(32|16)|\bv_pk_fma|atomic|scratch_', outputs_isa)


# ---------------------------------------------------------------------------------------------------------------------------------
# TaskOutputs
# ---------------------------------------------------------------------------------------------------------------------------------
def test_tables_broadcast_default_and_refuse():
    o = TaskOutputs(matrix=[[1.0, 0.0, 2.0], [0.0, -1.0, 0.5]], weights=[1.0, 2.0], target=0.5, hi=[np.inf, 3.0])
    t = o.tables(3)
    assert t['matrix'].dtype == F and t['matrix'].shape == (2, 3) and t['weight'].tolist() == [1, 2] and t['target'].tolist() == [[0.5, 0.5]]
    assert t['linear'].tolist() == [0, 0] and t['near'].tolist() == [0, 0] and t['lo'].tolist() == [-np.inf] * 2 and t['hi'].tolist() == [np.inf, 3.0]
    assert t['terminal'] is None
    one = TaskOutputs(matrix=[1.0, 2.0, 3.0], terminal_weights=4.0).tables(3)
    assert one['matrix'].tolist() == [[1, 2, 3]] and one['terminal'].tolist() == [4.0] and one['target'].tolist() == [[0.0]]
    per_step = TaskOutputs(matrix=np.ones((2, 3)), target=np.arange(8.0).reshape(4, 2))
    assert per_step.tables(3)['target'].shape == (4, 2) and per_step.tables(3, ref_rows=4)['target'][3].tolist() == [6, 7]
    ok = dict(matrix=np.ones((2, 3)))
    bad = [dict(matrix=None), dict(matrix=np.ones((17, 3))), dict(matrix=np.ones((2, 4))), dict(matrix=np.zeros((0, 3))), dict(matrix=[[np.nan, 0, 0]]),
           dict(matrix=[[np.inf, 0, 0]]), dict(ok, weights=-1.0), dict(ok, weights=np.nan), dict(ok, weights=[1.0, 2.0, 3.0]), dict(ok, target=np.inf),
           dict(ok, target=np.zeros((4, 3))), dict(ok, linear=np.nan), dict(ok, near=np.inf), dict(ok, lo=np.nan), dict(ok, hi=np.nan),
           dict(ok, lo=1.0, hi=0.0), dict(ok, terminal_weights=-1.0), dict(ok, terminal_weights=np.nan)]
    TaskOutputs(**ok).tables(3)
    TaskOutputs(**dict(ok, lo=1.0, hi=1.0)).tables(3)
    for kw in bad:
        with pytest.raises(ValueError):
            TaskOutputs(**kw).tables(3)
    with pytest.raises(ValueError):
        per_step.tables(3, ref_rows=5)
    with pytest.raises(ValueError):
        QuadraticTask(q=1.0, outputs=per_step).output_tables(3)                   # (a quadratic task has one row)
    with pytest.raises(ValueError):
        QuadraticTask(q=1.0, outputs='a matrix').output_tables(3)
    assert TrackingTask(reference=np.zeros((4, 3), F), outputs=per_step).output_tables(3)['target'].shape == (4, 2)


def test_the_tasks_carry_outputs_and_zones_may_name_them():
    o = TaskOutputs(matrix=np.ones((2, 3)))
    # `outputs` sits in front of `zones`, which stays the last field (tests/test_zones_cpu.py holds that)
    assert [f.name for f in dataclasses.fields(QuadraticTask)][-2:] == ['outputs', 'zones']
    assert [f.name for f in dataclasses.fields(TrackingTask)][-2:] == ['outputs', 'zones']
    q = QuadraticTask.to_target([1.0, 0.0, 0.0], outputs=o)
    t = TrackingTask.to_reference(np.zeros((2, 3), F), outputs=o)
    assert q.outputs is o and t.outputs is o and QuadraticTask().outputs is None and QuadraticTask().output_tables(3) is None
    assert 'outputs' not in q.tables(3, 1) and q.output_tables(3)['matrix'].shape == (2, 3)
    z = StateZones(axes=[[0, 4]], radius=1.0)
    assert dataclasses.replace(q, zones=z).zone_tables(3)['axis'].tolist() == [[0, 4, -1, -1]]
    for task in (dataclasses.replace(q, zones=StateZones(axes=[[0, 5]], radius=1.0)), QuadraticTask(q=1.0, zones=z)):
        with pytest.raises(ValueError):
            task.zone_tables(3)                                                   # past the outputs; no outputs at all


def test_quadratic_form_is_the_full_matrix_cost():
    rng = np.random.default_rng(0)
    O = 9
    B = rng.normal(size=(5, O))
    Q = B.T @ B                                                                   # rank 5
    g = rng.normal(size=O)
    o = TaskOutputs.quadratic_form(Q, g, terminal=2.0)
    t = o.tables(O)
    assert t['matrix'].shape == (5, O) and t['weight'].tolist() == [1.0] * 5 and t['terminal'].tolist() == [2.0] * 5
    s = rng.normal(size=(200, O))
    L = np.linalg.eigh(Q)
    want = np.einsum('ni,ij,nj->n', s - g, Q, s - g)
    Lm = o.matrix.astype(np.float64)
    got = ((s @ Lm.T - np.asarray(o.target, np.float64)) ** 2).sum(axis=1)
    assert np.abs(got - want).max() <= 1e-5 * np.abs(want).max()                  # (the rows are stored in float32)
    lam = L[0][::-1][:5]
    assert np.allclose((Lm ** 2).sum(axis=1), lam, rtol=1e-5)                     # sqrt(lambda_i) v_i, largest first
    # through the mirror: phi of a task with these outputs and q = 0 is the form
    tr = s.reshape(20, 10, O).astype(F)
    act = np.zeros((20, 9, 1), F)
    ret, _ = task_objective(tr, act, QuadraticTask(outputs=dataclasses.replace(o, terminal_weights=None)), 'cem')
    assert np.abs(-ret - want.reshape(20, 10)[:, 1:].sum(axis=1)).max() <= 1e-4 * np.abs(ret).max()
    per_step = TaskOutputs.quadratic_form(Q, rng.normal(size=(4, O)))
    assert np.asarray(per_step.target).shape == (4, 5)
    for bad in (np.ones((3, 4)), np.array([[1.0, 2.0], [0.0, 1.0]]), -np.eye(3), np.zeros((3, 3)), np.diag([1.0, -0.5, 1.0]), np.eye(17)):
        with pytest.raises(ValueError):
            TaskOutputs.quadratic_form(bad, np.zeros(bad.shape[0]))
    assert TaskOutputs.quadratic_form(np.eye(16), np.zeros(16)).tables(16)['matrix'].shape == (16, 16)
    with pytest.raises(ValueError):
        TaskOutputs.quadratic_form(np.eye(3), np.zeros(4))


def test_halfspaces_and_stack():
    hs = TaskOutputs.halfspaces([[1.0, 1.0, 0.0], [0.0, 1.0, -1.0]], [0.5, 2.0])
    t = hs.tables(3)
    assert t['hi'].tolist() == [0.5, 2.0] and t['lo'].tolist() == [-np.inf] * 2 and (t['weight'] == 0).all()
    qf = TaskOutputs.quadratic_form(np.diag([4.0, 0.0, 1.0]), [1.0, 0.0, -1.0], terminal=3.0)
    both = TaskOutputs.stack(qf, hs).tables(3)
    assert both['matrix'].shape == (4, 3) and both['weight'].tolist() == [1, 1, 0, 0] and both['hi'].tolist() == [np.inf, np.inf, 0.5, 2.0]
    assert both['terminal'].tolist() == [3, 3, 0, 0] and both['target'].shape == (1, 4) and both['target'][0, 2:].tolist() == [0, 0]
    np.testing.assert_array_equal(both['matrix'][2:], t['matrix'])
    stepped = TaskOutputs.stack(TaskOutputs(matrix=np.ones((1, 3)), target=np.arange(4.0)[:, None]), hs).tables(3)
    assert stepped['target'].shape == (4, 3) and stepped['target'][:, 0].tolist() == [0, 1, 2, 3] and stepped['terminal'] is None
    with pytest.raises(ValueError):
        TaskOutputs.stack(hs, TaskOutputs(matrix=np.ones((1, 4))))
    with pytest.raises(ValueError):
        TaskOutputs.stack(TaskOutputs(matrix=np.ones((9, 3))), TaskOutputs(matrix=np.ones((8, 3)))).tables(3)


# ---------------------------------------------------------------------------------------------------------------------------------
# the mirror
# ---------------------------------------------------------------------------------------------------------------------------------
def _cases():
    """task_cases.SHAPES x three variants x both base kinds x M = 1, 7, 16, clip on and off and zones on output axes on and off in
    turn; a per-step target of the outputs wherever the tracking base has more than one row; every threshold cleared."""
    for (O, A, H, rows, P) in oc.SHAPES:
        for vi, variant in enumerate(('cem', 'safe', 'cost')):
            for kind in ('quadratic', 'tracking'):
                for mi, M in enumerate(oc.COUNTS):
                    seed, clip, zoned = mi % 2, (vi + mi) % 2 == 0, (vi + mi + (kind == 'tracking')) % 2 == 0
                    tr, act = tc.random_case(O, A, H, rows, P, seed)
                    if kind == 'quadratic':
                        base, k0, prev, T = tc.task_for(O, A, seed, clip), 0, None, None
                    else:
                        T, k0 = tk.clock_cases(H)[(vi + mi) % 5]
                        base, prev = tk.tracking_task_for(O, A, T, seed, clip), tk.prev_action_for(A, seed)
                    out = oc.random_outputs(O, M, seed, T=T if T and T > 1 else None, terminal=kind == 'tracking')
                    task = oc.with_outputs(base, out, oc.output_zones(O, M, seed) if zoned else None)
                    oc.clear_output_thresholds(tr, task, k0)
                    yield (O, variant, kind, M, zoned, clip), task, tr, act, variant, k0, prev


def test_mirror_against_float64():
    """The mirror against the contract in float64 (output_cases.outputs_f64).  No comparison operand lies within 1e-4 of its threshold
    (asserted), so cost bytes and done steps are EQUAL; the bar on the returns is twice output_cases.MIRROR_ERROR_MEASURED, the largest
    distance relative to max(1, |return|) measured over these cases on the CPU."""
    worst, seen = 0.0, set()
    for what, task, tr, act, variant, k0, prev in _cases():
        r64, c64, d64, margin = oc.outputs_f64(tr, act, task, variant, k0, prev)
        r32, c32, d32 = _objective(task, tr, act, variant, k0, prev, return_done=True)
        assert margin > tc.NEAR, (what, margin)
        assert r32.dtype == F and np.array_equal(d32, d64), what
        if variant == 'cem':
            assert c32 is None and c64 is None
        else:
            assert c32.dtype == np.uint8 and np.array_equal(c32, c64), what
            if tr.shape[0] > 3:                                                   # the outputs' bounds (and zones) reach the cost bytes
                assert c64.sum() > _objective(dataclasses.replace(task, outputs=None, zones=None), tr, act, variant, k0, prev)[1].sum(), what
        seen.add(what[1:])
        worst = max(worst, float((np.abs(r32.astype(np.float64) - r64) / np.maximum(1.0, np.abs(r64))).max()))
    print('outputs mirror against float64: largest relative distance %.3g' % worst)
    assert len({s[:3] for s in seen}) == 18 and {s[3] for s in seen} == {True, False} == {s[4] for s in seen}
    assert worst <= 2 * oc.MIRROR_ERROR_MEASURED, worst
    assert worst > 0.5 * oc.MIRROR_ERROR_MEASURED, worst                          # (the recorded figure is this test's own)


@pytest.mark.parametrize('kind', ['quadratic', 'tracking'])
def test_without_outputs_and_with_idle_outputs_the_bits_are_the_base_tasks(kind):
    """outputs None runs the code of a task without; outputs with no weight, linear term or near weight and infinite bounds add
    (+0 - +-0) = +0 to partial sums that are never -0, and set no byte: every bit the same, with and without zones."""
    for (O, A, H, rows, P) in oc.SHAPES:
        for variant in ('cem', 'safe', 'cost'):
            tr, act = tc.random_case(O, A, H, rows, P, 1)
            if kind == 'quadratic':
                base, k0, prev = tc.task_for(O, A, 1, True), 0, None
                tc.craft(tr, base, boundaries=False)
            else:
                base, k0, prev = tk.tracking_task_for(O, A, H + 1, 1, True), 1, tk.prev_action_for(A)
                tk.craft(tr, act, base, k0, prev, boundaries=False)
            assert base.outputs is None
            idle = TaskOutputs(matrix=np.random.default_rng(O).uniform(-1, 1, (7, O)).astype(F), target=np.arange(7.0))
            for zones in (None, zc.random_zones(O, 1)):
                want = _objective(dataclasses.replace(base, zones=zones), tr, act, variant, k0, prev, return_done=True)
                _same(_objective(oc.with_outputs(base, idle, zones), tr, act, variant, k0, prev, return_done=True), want)


@pytest.mark.parametrize('kind', ['quadratic', 'tracking'])
@pytest.mark.parametrize('shape', oc.SHAPES[1:], ids=lambda s: 'O%d' % s[0])
def test_mirror_crafted_rows(shape, kind):
    """What the contract says ON the thresholds (the kernel is held to the mirror bit for bit on the GPU)."""
    O, A, H, rows, P = shape
    base, g, k0, prev = zc.crafted_base(O, A, kind, H)
    task, tr, act, n = oc.crafted_case(base, O, A, H, P, g)
    b = zc.craft_features(O)
    y = output_terms(tr, task.output_tables(O))
    clean = ~np.isnan(tr).any(axis=2)
    np.testing.assert_array_equal(y[clean][:, :5].view(U), tr[clean][:, b:b + 5].view(U))      # a unit row IS its feature, bit for bit
    assert (b >= 64) == (O > 64)                                                  # at O = 100 the rows read the second quad
    ret_e, _ = _objective(task, tr, act, 'cem', k0, prev)
    ret_s, cost_s, first = _objective(task, tr, act, 'safe', k0, prev, return_done=True)
    ret_c, cost_c = _objective(task, tr, act, 'cost', k0, prev)
    for costs in (cost_s, cost_c):
        assert costs[:, n['on_hi']].sum() == 0 and costs[1, n['ulp_above_hi']] == 1 and costs[:, n['ulp_above_hi']].sum() == 1
        assert costs[1, n['zone_exactly']] == 1 and costs[:, n['zone_ulp_outside']].sum() == 0
        assert costs[0, n['violation_at_0']] == 1 and costs[:, n['violation_at_H']].sum() == 0     # (no step's cost reads s_H)
        assert costs[:, n['nan_under_zero_column']].sum() == 0 and costs[:, n['calm']].sum() == 0
    # near through the output's near weight alone: exactly R2 is near (the episode ends at step 0), one ulp beyond is not
    assert first[n['near_by_output_exactly']] == 0 and first[n['near_by_output_ulp_outside']] == H and first[n['calm']] == H
    # a violation after near: masked by done in 'safe', counted in 'cost'
    assert first[n['violation_after_near']] == 0 and cost_s[:, n['violation_after_near']].sum() == 0 and cost_c[2, n['violation_after_near']] == 1
    # the terminal weight: 5 x 0.25 at s_H on a tracking base, the weight's 1 x 0.25 on a quadratic one and at s_{H-1}
    gap = float(ret_c[n['deviation_before_H']]) - float(ret_c[n['deviation_at_H']])
    assert abs(gap - (1.0 if kind == 'tracking' else 0.0)) < 1e-3, gap
    # 0 x NaN: the state's outputs are NaNs, phi with them, and the unclipped reward is fmaxf(NaN, -inf) = -inf as for a NaN feature
    assert np.isnan(y[n['nan_under_zero_column'], 1]).all() and ret_e[n['nan_under_zero_column']] == -np.inf and np.isfinite(ret_e[n['calm']])
    # the zone on two outputs pays its margin's hinge: (0.75^2 - dist2) x 2
    free = dataclasses.replace(task, zones=dataclasses.replace(task.zones, penalty=0.0))
    r_free = _objective(free, tr, act, 'cost', k0, prev)[0]
    assert r_free[n['zone_exactly']] - ret_c[n['zone_exactly']] == pytest.approx(2.0 * (0.5625 - 0.25), rel=1e-3)
    assert r_free[n['calm']].view(U) == ret_c[n['calm']].view(U)


def test_sixteen_output_slots_are_added_pairwise():
    """Sixteen outputs whose terms span six decades, on a base task without weights: phi is the pairwise tree's sum of the sixteen
    slot values, and a left-to-right sum of the same slots differs."""
    for O in (57, 100):
        tr, act = tc.random_case(O, 2, 7, 48, 3, 2)
        tr = np.clip(tr, -2.0, 2.0)
        out = oc.sixteen_outputs(O)
        ot = out.tables(O)
        y = output_terms(tr, ot)
        slots = ot['weight'] * (y * y) - ot['linear'] * y
        assert slots[slots > 0].max() / slots[slots > 0].min() > 1e6
        tree = slots
        for _ in range(4):
            tree = tree[..., 0::2] + tree[..., 1::2]
        left = np.zeros(tree[..., 0].shape, F)
        for m in range(16):
            left = left + slots[..., m]
        assert (left.view(U) != tree[..., 0].view(U)).mean() > 0.3
        ret, _ = task_objective(tr, np.zeros_like(act), QuadraticTask(outputs=out), 'cem')
        want = np.zeros(tr.shape[0], F)
        for t in range(7):
            want = want + (-tree[:, t + 1, 0])
        np.testing.assert_array_equal(ret.view(U), want.view(U))


def test_the_closed_loop_reference_figures_are_the_references():
    """The constants of tests/test_gpu_task_outputs.py's closed loops, measured here with the NumPy CEM of
    output_cases.reference_closed_loop over seeds 0 .. 4.  At the wall: with the half-space it executes no state beyond the wall and
    ends within REFERENCE_WALL_WORST_DISTANCE of the wall's closest point to the target; without, it crosses the wall on every seed.
    At the thin diagonal obstacle: with the outputs and the zone on them it executes no state inside and ends within
    REFERENCE_ZONE_WORST_STAGE_COST of the set-point; without, it runs through on every seed."""
    wall = [oc.reference_closed_loop(s, oc.wall_task(True), 'safe') for s in range(5)]
    free = [oc.reference_closed_loop(s, oc.wall_task(False), 'safe') for s in range(5)]
    dist = [float(np.linalg.norm(ex[-1, :2].astype(np.float64) - oc.CLOSEST)) for ex in wall]
    print('wall reference: beyond', [oc.beyond_wall(ex) for ex in wall], 'without', [oc.beyond_wall(ex) for ex in free], 'final distance', dist)
    assert all(oc.beyond_wall(ex) == 0 for ex in wall) and all(oc.beyond_wall(ex) > 0 for ex in free)
    assert 0.9 * oc.REFERENCE_WALL_WORST_DISTANCE < max(dist) <= oc.REFERENCE_WALL_WORST_DISTANCE
    zone = [oc.reference_closed_loop(s, oc.zone_task(True)) for s in range(5)]
    thru = [oc.reference_closed_loop(s, oc.zone_task(False)) for s in range(5)]
    cost = [zc.stage_cost(ex[-1]) for ex in zone]
    print('zone reference: inside', [oc.inside_zone(ex) for ex in zone], 'without', [oc.inside_zone(ex) for ex in thru], 'final stage cost', cost)
    assert all(oc.inside_zone(ex) == 0 for ex in zone) and all(oc.inside_zone(ex) > 0 for ex in thru)
    assert 0.9 * oc.REFERENCE_ZONE_WORST_STAGE_COST < max(cost) <= oc.REFERENCE_ZONE_WORST_STAGE_COST
    assert oc.LOOP['N'] <= 256 and oc.LOOP['H'] <= 15 and oc.LOOP['I'] <= 4 and oc.LOOP['steps'] <= 80
