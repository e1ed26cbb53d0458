"""Option combinations on the device: csrc/cem_plan_options.h says which combinations a handle admits, this file says what
an admitted combination COMPUTES.

tests/composed_cases.py generates 48 handles — every pair of the ten options forced on once, four handles with everything on — and holds
the one composed restatement of a plan, as stage functions.  Each case runs two consecutive stepwise plans in Philox mode (so that mixed
noise is live, and across-plans carry and warm start have a second plan to act on) and checks every stage of every iteration against
the restatement on the device's OWN inputs of that stage (teacher forcing: a near-tie never excuses a mismatch), in the style of
tests/test_gpu_fuzz.py::test_random_shape_whole_plan_teacher_forced:
    init, noise, the reported rollout path, candidates (both layouts), rollout, scores, select and refit, keep, track, plan_end
with everything beyond the leading n[it] entries of the per-candidate arrays poisoned in front of both launches.  A graph handle of the same
case then runs the same two calls as whole plans and must return the same bits: the form that ships is tied to the form just verified.
Every bar below is one an existing test uses for the same stage (named where it is applied)."""
import os

import numpy as np
import pytest

from oracle import cem_oracle as o
from ethz_safe_learning_amd.planner import task_objective
from tests import composed_cases as cp
from tests import cost_cases
from tests import decay_cases as dc
from tests import helpers as hp
from tests import lean_cases as lc
from tests.test_gpu_parity import ATOL

pytestmark = pytest.mark.gpu
# CEM_FUZZ_SCALE=n multiplies the number of seeds (tests/test_gpu_fuzz.py): later rounds force the same pairs on other shapes
SCALE = int(os.environ.get('CEM_FUZZ_SCALE', '1'))
F, U = np.float32, np.uint32
SEED, CALL = cp.PLAN_SEED, cp.PLAN_CALL


def _torch():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch


def _np(t):
    return t.cpu().numpy().copy()


def _bits(a, b, what=''):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    np.testing.assert_array_equal(a.view(U) if a.dtype == F else a, b.view(U) if b.dtype == F else b, err_msg=what)


def _score_bits(x):
    """The bits of a best score with -0.0 read as +0.0: the two are one value to every select, and "the best score of a plan whose best
    candidate scored -0.0 may be reported as +0.0" (include/cem_mpc.h, select_mode) — the cost objective's best score is often that zero."""
    return (F(x) + F(0.0)).view(U)


def _same_block(got, want, what=''):
    """Field for field, floats by their bits (tests/test_gpu_plan_readout.py)."""
    assert (got.candidate, got.iteration, got.flags) == (want.candidate, want.iteration, want.flags), (what, got, want)
    assert _score_bits(got.score) == _score_bits(want.score), (what, got.score, want.score)
    _bits(got.sequence, want.sequence, '%s: sequence' % what)
    _bits(got.particle_returns, want.particle_returns, '%s: particle_returns' % what)
    np.testing.assert_array_equal(got.cost_counts, want.cost_counts, err_msg='%s: cost_counts' % what)


def _planner(case, use_graph=False, n=None, options=True):
    """A handle of the case with its options applied through the setters (every one must answer OK: a refusal raises), or a
    never-optioned handle created with n_samples = n."""
    _torch()
    pb = cp.problem(case)
    over = dict(use_graph=use_graph)
    if n is not None:
        over['N'] = n
    _, pcfg = hp.configs(pb, **cp.config_kwargs(case, **over))
    pl = hp.make_planner(pb, pcfg)
    if options:
        cp.apply_options(pl, case)
    return pl


def _check_rollout(case, ref, pl, plain, it, call, acts, ret, costs, what):
    """The rollout against the fp64 oracle on the device's own sample, with the model noise of a never-optioned handle created with
    n_samples = n[it] (a scheduled iteration IS that handle's)."""
    pb, n, P, H = ref.pb, ref.n[it], case.P, case.H
    sp = pb['scorer']
    em = _np(plain.fill_noise(SEED, call)[1][it])                                  # [H, P n, O]
    w64 = o.cast_weights(pb['weights'], np.float64)
    if case.opt.task is not None:
        # the trajectories the task scores: the 5e-6 bar of tests/test_gpu_fuzz.py::test_random_shape_unfold_and_objective_ops
        s0 = np.tile(pb['state'].astype(np.float64), (P * n, 1))
        ref64 = o.unfold_sequences(s0, np.tile(acts.astype(np.float64), (P, 1, 1)), w64, o.member_of_rows(P * n, case.E), pb['inputs_min'],
                                   pb['inputs_max'], em.astype(np.float64), ref.ocfg.scale_features, ref.ocfg.sampling_propagation)
        traj = _np(pl.task_trajectories())[:P * n]
        err = float(np.abs(traj - ref64).max())
        print('%s: task trajectories max |gpu - f64| = %.3g (scale %.3g)' % (what, err, float(np.abs(ref64).max())))
        assert err <= 5e-6 * max(1.0, np.abs(ref64).max()), (what, err)
        return
    _, traj64 = o.candidate_scores(pb['state'].astype(np.float64), acts.astype(np.float64), w64, pb['inputs_min'], pb['inputs_max'], em,
                                   ref.cfg_it(it), sp, return_traj=True)
    if case.variant == 'cost':
        # the un-masked cost bytes (the returns a cost handle's rollout also writes mean nothing): exact on every (step, row) clear of a cost
        # threshold, hp.NEAR as tests/helpers.assert_scores_match_oracle takes it
        ok = cost_cases.cost_margins(traj64, sp) > hp.NEAR
        np.testing.assert_array_equal(costs.reshape(H, P * n)[ok], cost_cases.cost_bytes(traj64, sp)[ok].astype(np.uint8), err_msg=what)
        return
    # the particle-mean objective of the device's own returns and cost bytes against the oracle's: hp.assert_scores_match_oracle at ATOL of
    # tests/test_gpu_parity.py, near-threshold candidates by their admissible outcomes (tests/test_gpu_fuzz.py, tests/test_gpu_lean_edges.py)
    plain_ref = cp.Reference(case._replace(opt=cp.NOTHING._replace(schedule=case.opt.schedule)))
    derived = plain_ref.scores(it, ret, costs)
    err, n_near, n_flip = hp.assert_scores_match_oracle(derived, traj64, P, n, sp, case.variant, cp.POST, ATOL, what)
    print('%s: max |gpu - f64| = %.3g; %d of %d candidates near a threshold (%d flipped)' % (what, err, n_near, n, n_flip))
    if case.variant == 'safe':
        # SafeCemMpc's done-masked cost bytes of the clear rows, exactly (tests/test_gpu_lean_edges.py)
        row_ok = o.threshold_margins(traj64, sp) > 1e-4
        ref_costs, _ = lc.masked_costs_and_first_goal(traj64, sp)
        np.testing.assert_array_equal(costs.reshape(H, P * n).astype(np.float64)[:, row_ok], ref_costs[:, row_ok], err_msg=what)


def _run_case(case, where):
    ref = cp.Reference(case)
    pb, opt, I, H, A, P = ref.pb, case.opt, case.I, case.H, case.A, case.P
    pf, psft = dc.pad_layout(case)
    handles, plains, results = [], {}, []
    try:
        pl = _planner(case)
        handles.append(pl)
        arr = hp.Arrays(pl, case)
        for plan in range(2):
            call = CALL + plan
            where.update(plan=plan, it=-1, stage='init')
            carry = pl.carry()
            store = pl.elite_store()[0] if opt.keep is not None else None          # the previous plan's last kept elites
            block = pl.plan_readout() if opt.readout else None
            xi = _np(pl.fill_noise(SEED, call)[0])                                  # the white streams, [I, N, H, A]
            pl.plan_begin(pb['state'], seed=SEED, call=call)
            mu_w, sg_w, st = ref.init(plan, carry, store)
            assert carry[2] == (plan > 0)
            ms = _np(pl.mu_sigma())
            _bits(ms[0], mu_w, 'mu of iteration 0'); _bits(ms[1], sg_w, 'sigma of iteration 0')
            where.update(stage='noise')
            eps = xi
            if opt.noise is not None:
                eps = np.asarray(pl.action_noise_tensor())                          # the handle's own tensor: the sampler is held to IT below
                _bits(eps, ref.action_noise(xi), 'mix_noise of the white streams')  # by bits: tests/test_gpu_colored_noise.py
            best, best_score, ran, decisive = np.zeros(A, F), F(-np.inf), 0, True
            for it in range(I):
                n = ref.n[it]
                what = '%s plan %d iteration %d' % (case.name, plan, it)
                where.update(it=it, stage='path')
                if n not in plains:
                    plains[n] = _planner(case, n=n, options=False)
                    handles.append(plains[n])
                plain = plains[n]
                ip = pl.iteration_plan(it)
                forced = cp.generic_forced(case, it)
                assert ip['n_samples'] == n and ip['rollout_path'] == ('generic' if forced else plain.rollout_path()), (ip, forced, plain.rollout_path())
                if cp.lean_eligible(case):
                    assert plain.rollout_path() == 'lean' and ip['rollout_path'] == ('generic' if forced else 'lean'), (ip, forced)
                ms = _np(pl.mu_sigma())
                where.update(stage='poison (rollout)')
                arr.poison(n)
                pl.plan_rollout(it)
                arr.check(n, what + ' rollout')
                where.update(stage='candidates')
                acts = arr.get('actions', n).reshape(n, H, A)
                _bits(acts, ref.candidates(it, ms[0], ms[1], eps[it], st, plan), 'actions')
                pad = arr.get('act_pad', n).reshape(n, H, pf)
                if ip['rollout_path'] == 'generic':                                 # (the lean kernels draw in place and keep no padded copy)
                    _bits(pad[:, :, psft:psft + A], acts, 'the padded quads at the action words')
                rest = np.ones(pf, bool)
                rest[psft:psft + A] = False
                assert not pad[:, :, rest].view(U).any(), 'a padding word is not zero'
                ret = arr.get('returns', n)
                costs = arr.get('costs', n, np.uint8) if ref.has_costs else None
                where.update(stage='rollout')
                if opt.task is not None:
                    # returns and cost bytes ARE task_objective on the device's own trajectories and sample (tests/test_gpu_task_scorer.py)
                    want_ret, want_costs = task_objective(_np(pl.task_trajectories())[:P * n], acts, opt.task, case.variant)
                    _bits(ret, want_ret, 'task returns')
                    if ref.has_costs:
                        _bits(costs, want_costs.reshape(-1), 'task cost bytes')
                if case.precision != 'bf16':
                    _check_rollout(case, ref, pl, plain, it, call, acts, ret, costs, what)
                where.update(stage='scores')
                scores = arr.get('scores', n)
                # by bits on every objective: the lower tail (tests/test_gpu_risk_objective.py), the budget encoding
                # (tests/test_gpu_cost_budget.py), the cost objective (tests/test_gpu_cost_objective.py) and the particle mean with its Beta
                # filter (tests/test_gpu_task_scorer.py _restated_scores, tests/test_gpu_cost_budget.py)
                _bits(scores, ref.scores(it, ret, costs), 'scores')
                where.update(stage='poison (select)')
                arr.poison(n)
                pl.plan_select(it)
                arr.check(n, what + ' select')
                where.update(stage='select')
                elite = _np(pl.elite_idx())
                mu_w, sg_w, best, best_score, elite_w, stop, mean_sigma = ref.select(it, scores, acts, ms[0], ms[1], best, best_score)
                np.testing.assert_array_equal(np.sort(elite), elite_w, err_msg='the elite set')
                got = _np(pl.mu_sigma())
                # mu / sigma live on the scale of the Box (+-100 when it is unbounded), and a dimension whose elites all hold one value has a
                # standard deviation of pure rounding noise, of the order sqrt(k) eps |c|: both allowances are those of
                # tests/test_gpu_fuzz.py::test_random_shape_whole_plan_teacher_forced, whose rtol / atol the uniform refit takes; the softmax
                # refit takes the rtol / atol of tests/test_gpu_population_decay.py::test_with_the_softmax_refit (a unit Box) on that scale
                amag = max(1.0, float(np.abs(ref.ub).max()))
                noise_floor = 4 * 1.2e-7 * float(np.abs(mu_w).max()) * np.sqrt(case.k)
                rt_mu, rt_sg, at = (2e-5, 2e-4, 2e-6) if opt.tau > 0 else (1e-5, 2e-5, 1e-6)
                print('%s: refit %s |mu err| %.3g |sigma err| %.3g box scale %.3g noise floor %.3g' % (
                    what, 'softmax' if opt.tau > 0 else 'uniform', np.abs(got[0] - mu_w).max(), np.abs(got[1] - sg_w).max(), amag, noise_floor))
                np.testing.assert_allclose(got[0], mu_w, rtol=rt_mu, atol=at * amag, err_msg='mu')
                np.testing.assert_allclose(got[1], sg_w, rtol=rt_sg, atol=at * amag + noise_floor, err_msg='sigma')
                if opt.keep is not None:
                    where.update(stage='keep')
                    st, count = pl.elite_store()
                    assert count == opt.keep.m
                    _bits(st, ref.keep(scores, elite, acts), 'keep_elites')
                if opt.readout:
                    where.update(stage='track')
                    block = ref.track(block, it, it + 1, best_score, scores, elite, acts, ret, costs)
                    _same_block(pl.plan_readout(), block, 'track_best')
                ran += 1
                # the stop rule compares mean(sigma) with the threshold: only decisive margins are asserted (the teacher-forced test's 1e-5)
                margin = abs(mean_sigma - case.thr)
                if margin <= 1e-5:
                    decisive = False
                    break
                if stop:
                    break
            where.update(it=-1, stage='plan_end')
            a, s, n_it = pl.plan_end()
            if decisive:
                assert n_it == ran, (n_it, ran)
                _bits(a, ref.finish(best, pl.output_noise(SEED, call)), 'action')
                assert _score_bits(s) == _score_bits(best_score), (s, best_score)
            results.append((a, s, n_it))
        where.update(plan=-1, stage='graph')
        pg = _planner(case, use_graph=True)
        handles.append(pg)
        for plan in range(2):
            a, s, n_it = pg.plan(pb['state'], seed=SEED, call=CALL + plan)
            _bits(a, results[plan][0], 'graph plan %d: action' % plan)
            assert F(s).view(U) == F(results[plan][1]).view(U) and n_it == results[plan][2], (plan, s, n_it, results[plan])
            assert pg.graph_status() == 'graph'
    finally:
        for h in handles:
            h.close()


def _run(case):
    where = dict(plan=-1, it=-1, stage='setup')
    try:
        _run_case(case, where)
    except Exception as e:
        raise AssertionError('plan %(plan)d, iteration %(it)d, stage %(stage)s' % where + '\n%r\n%s: %s' % (case, type(e).__name__, e)) from e


@pytest.mark.parametrize('seed', range(cp.N_SEEDS * SCALE))
def test_option_combination_teacher_forced(seed):
    _run(cp.case_for(seed))
