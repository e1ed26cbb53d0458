"""Plan read-out (cem_planner_set_plan_readout) on the device.

The tracker has an exact reference that costs nothing: planner.track_best is comparisons, copies and integer counts, and everything it
reads — the control block's iters and best_score, the scores the select ranked, the elite list, the sample, `ret`, the cost bytes — can be
read back from the workspace after every launch.  So the stepwise form is checked launch by launch over tests/readout_cases.py (1), the
whole-plan invariants hang off the same run (2), and the rest — the plan forms, batch handles, early stop, the oracle, off is off, the
other settings, the policies — off that."""
import ctypes

import numpy as np
import pytest

from oracle import cem_oracle as o
from ethz_safe_learning_amd import BatchCemPlanner, _capi
from ethz_safe_learning_amd.planner import track_best
from tests import helpers as hp
from tests import readout_cases as rc

pytestmark = pytest.mark.gpu

F, U = np.float32, np.uint32
INVALID_ARG, UNSUPPORTED, STATE = 1, 2, 7
SEED, CALL = rc.PLAN_SEED, rc.PLAN_CALL
I = rc.I
IDS = [c.name for c in rc.CASES]
CTRL_BYTES, CTRL_ITERS, CTRL_BEST = 680, 20, 24          # cem_device.h CtrlBlock: its size, and where iters and best_score stand in it


def _torch():
    import torch
    assert torch.cuda.is_available(), 'gpu tests need an MI355X'
    return torch


def _np(t):
    return t.cpu().numpy().copy()


def _bits(a, b, what=''):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    np.testing.assert_array_equal(a.view(U) if a.dtype == F else a, b.view(U) if b.dtype == F else b, err_msg=what)


def _same_block(got, want, what=''):
    """Field for field, floats by their bits."""
    assert (got.candidate, got.iteration, got.flags) == (want.candidate, want.iteration, want.flags), (what, got, want)
    assert F(got.score).view(U) == F(want.score).view(U), (what, got.score, want.score)
    _bits(got.sequence, want.sequence, '%s: sequence' % what)
    _bits(got.particle_returns, want.particle_returns, '%s: particle_returns' % what)
    np.testing.assert_array_equal(got.cost_counts, want.cost_counts, err_msg='%s: cost_counts' % what)


def _planner(case, monkeypatch, on=True, **over):
    """A handle of the case, created under the case's CEM_FORCE_ROLLOUT, its population schedule set, the read-out on unless on=False."""
    _torch()
    if case.force:
        monkeypatch.setenv('CEM_FORCE_ROLLOUT', case.force)
    else:
        monkeypatch.delenv('CEM_FORCE_ROLLOUT', raising=False)
    pb = rc.problem(case)
    _, pcfg = hp.configs(pb, **rc.config_kwargs(case, **over))
    pl = hp.make_planner(pb, pcfg)
    monkeypatch.delenv('CEM_FORCE_ROLLOUT', raising=False)
    if case.population:
        pl.set_population_schedule(case.population)
    if on:
        pl.set_plan_readout(True)
    return pb, pl


def _ctrl(pl, problem=0):
    """(iters, best_score) of the problem's control block, the workspace's first array (cem_capi.hip make_layout)."""
    pl.synchronize()
    raw = _np(pl._ws_view[problem * CTRL_BYTES:(problem + 1) * CTRL_BYTES])
    return int(raw[CTRL_ITERS:CTRL_ITERS + 4].view(np.int32)[0]), raw[CTRL_BEST:CTRL_BEST + 4].view(F)[0]


def _launch_inputs(pl, case, it):
    """What launch `it` of the tracker read: everything track_best takes behind (block, it)."""
    iters, best = _ctrl(pl)
    costs = _np(pl.costs()).reshape(-1) if rc.has_costs(case) else None
    return dict(iters=iters, best_score=best, scores=_np(pl.scores_global()), elite_idx=_np(pl.elite_idx()), actions=_np(pl.actions()),
                ret=_np(pl.returns()).reshape(-1), costs=costs, n=rc.population(case, it))


def _status(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except _capi.CemError as e:
        return e.status
    return 0


def _fp32_mean(returns):
    acc = F(0)
    for r in returns:
        acc = F(acc + r)
    return F(acc / F(len(returns)))


# ------------------------------------------------------------------------------------------------- 1, 2, 3: launch by launch, invariants, plan forms
@pytest.mark.parametrize('case', rc.CASES, ids=IDS)
def test_tracker_launch_by_launch_and_the_invariants_of_the_plan(case, monkeypatch):
    """Teeth.  After every select call of a stepwise plan the block equals track_best on what the workspace holds; at the plan's end
    sequence[0] is the returned action and score the returned score (noise_stddev = 0), on 'cem' the score is the fp32 mean of the
    particle returns, and the sequence is the candidate's row of the oracle's sample on the dumped Philox stream.  The eager and the
    captured plan leave the same block; rollout_path / rollout_form are what a handle without the read-out reports."""
    pb, off = _planner(case, monkeypatch, on=False)
    pb, pl = _planner(case, monkeypatch)
    assert pl.plan_readout_enabled() and not off.plan_readout_enabled()
    assert pl.rollout_path() == off.rollout_path()
    if case.lean or case.force:
        assert pl.rollout_path() == ('generic' if case.force else 'lean')
    assert [pl.rollout_form(it) for it in range(I)] == [off.rollout_form(it) for it in range(I)]
    assert pl.launches_per_iteration() == off.launches_per_iteration() + 1
    _same_block(pl.plan_readout(), rc.empty(case), 'before any plan')
    lb, ub, _, _ = o.sampling_params(pb['low'], pb['high'])
    ea = _np(pl.fill_noise(seed=SEED, call=CALL)[0])
    pl.plan_begin(pb['state'], seed=SEED, call=CALL)
    block, drawn = pl.plan_readout(), []
    for it in range(I):
        ms = _np(pl.mu_sigma())
        n = rc.population(case, it)
        drawn.append(o.sample_actions(ms[0], ms[1], lb, ub, ea[it][:n]))
        pl.plan_rollout(it)
        pl.plan_select(it)
        got = pl.plan_readout()                                                   # (readable inside a stepwise plan)
        inp = _launch_inputs(pl, case, it)
        assert inp['iters'] == it + 1
        block = track_best(block, it, **inp)
        _same_block(got, block, 'iteration %d' % it)
        assert got.flags == 0 and got.candidate >= 0 and got.iteration <= it
    a, s, n_it = pl.plan_end()
    final = pl.plan_readout()
    _same_block(final, block, 'after plan_end')
    assert n_it == I
    _bits(final.sequence[0], a, 'sequence[0] is the returned action')
    assert F(final.score).view(U) == F(s).view(U)
    if case.variant == 'cem':
        assert _fp32_mean(final.particle_returns).view(U) == F(s).view(U), (final.particle_returns, s)
        assert (final.cost_counts == -1).all()
    else:
        assert ((final.cost_counts >= 0) & (final.cost_counts <= case.P)).all()
    _bits(final.sequence, drawn[final.iteration][final.candidate], 'the sequence is the candidate\'s row of that iteration\'s sample')
    # the whole-plan forms
    r = off.plan(pb['state'], seed=SEED, call=CALL)
    _bits(r[0], a, 'the read-out changes no result bit'); assert F(r[1]).view(U) == F(s).view(U) and r[2] == n_it
    pb, pe = _planner(case, monkeypatch)
    r = pe.plan(pb['state'], seed=SEED, call=CALL)
    _bits(r[0], a, 'eager: action'); assert F(r[1]).view(U) == F(s).view(U)
    _same_block(pe.plan_readout(), final, 'eager')
    assert pe.graph_status() == 'eager'
    pb, pg = _planner(case, monkeypatch, use_graph=True)
    for rep in range(2):                                                          # captured, then replayed
        r = pg.plan(pb['state'], seed=SEED, call=CALL)
        _bits(r[0], a, 'graph: action')
        _same_block(pg.plan_readout(), final, 'graph, plan %d' % rep)
        assert pg.graph_status() == 'graph'
    for p in (off, pl, pe, pg):
        p.close()


@pytest.mark.parametrize('case', rc.CASES, ids=IDS)
def test_tracker_on_adversarial_scores(case, monkeypatch):
    """Teeth.  The launch-by-launch run again with scores_local overwritten between rollout and select, in iteration 0 and in iteration
    1 (the same vector: an equal best score later in the plan is no update): ties at the maximum and across the k-th place, both zeros,
    NaN, the infinities."""
    torch = _torch()
    pb, pl = _planner(case, monkeypatch)
    updated = 0
    for name, vec in rc.adversarial_scores(case).items():
        pl.plan_begin(pb['state'], seed=SEED, call=CALL)
        block = pl.plan_readout()
        for it in range(2):
            pl.plan_rollout(it)
            pl.synchronize()
            with pl.stream_context():
                pl.scores_local(sync=False).copy_(torch.from_numpy(vec))
            pl.plan_select(it)
            got = pl.plan_readout()
            inp = _launch_inputs(pl, case, it)
            _bits(inp['scores'], vec, name)
            block = track_best(block, it, **inp)
            _same_block(got, block, '%s iteration %d' % (name, it))
            assert got.flags == 0, name
            if got.iteration == it:
                # the winner is an elite of exactly the best score, and no elite of that score has a lower index
                n = inp['n']
                same = [int(e) for e in inp['elite_idx'] if vec[e] == got.score]
                assert got.candidate == min(same) and got.candidate < n, (name, it, got.candidate, same)
        updated += got.candidate >= 0
        if name == 'tie_at_the_maximum' and not case.population:
            top = np.nonzero(vec == vec.max())[0]
            assert got.candidate == top.min() and got.iteration == 0 and top.size >= 3
        pl.plan_end()
    assert updated >= 5                                                           # (the vectors are live: most of them name a winner)
    pl.close()


@pytest.mark.parametrize('use_graph', [False, True])
def test_the_lean_and_the_forced_generic_plan_leave_the_same_block(use_graph, monkeypatch):
    lean, forced = rc.BY_NAME['lean_one_quad'], rc.BY_NAME['forced_generic']
    pb, pl = _planner(lean, monkeypatch, use_graph=use_graph)
    pb, pf = _planner(forced, monkeypatch, use_graph=use_graph)
    assert (pl.rollout_path(), pf.rollout_path()) == ('lean', 'generic')
    for j in range(2):
        a = pl.plan(pb['state'], seed=SEED, call=CALL + j)
        b = pf.plan(pb['state'], seed=SEED, call=CALL + j)
        _bits(a[0], b[0], 'action'); assert F(a[1]).view(U) == F(b[1]).view(U) and a[2] == b[2]
        got = pl.plan_readout()
        _same_block(got, pf.plan_readout(), 'plan %d' % j)
        assert got.candidate >= 0 and got.flags == 0
    pl.close(); pf.close()


def test_early_stop_leaves_the_block_of_the_last_counted_iteration(monkeypatch):
    case = rc.BY_NAME['lean_one_quad']
    pb, pl = _planner(case, monkeypatch)
    sig = []
    pl.plan_begin(pb['state'], seed=SEED, call=CALL)
    for it in range(I):
        pl.plan_rollout(it)
        pl.plan_select(it)
        sig.append(float(_np(pl.mu_sigma())[1].mean(dtype=F)))
    pl.plan_end()
    pl.close()
    assert sig[1] < sig[0], sig
    thr = 0.5 * (sig[0] + sig[1])                                                 # the select of iteration 1 stops the plan
    pb, pl = _planner(case, monkeypatch, thr=thr)
    pl.plan_begin(pb['state'], seed=SEED, call=CALL)
    block = pl.plan_readout()
    for it in range(2):
        pl.plan_rollout(it)
        pl.plan_select(it)
        block = track_best(block, it, **_launch_inputs(pl, case, it))
    want = pl.plan_readout()                                                      # the select that set `done` was still tracked
    _same_block(want, block, 'the stopping iteration')
    pl.plan_rollout(2)                                                            # rollout, select: both leave at once; the tracker's gate holds
    pl.plan_select(2)
    assert _ctrl(pl)[0] == 2
    _same_block(pl.plan_readout(), want, 'after the iteration that did not run')
    a, s, n_it = pl.plan_end()
    assert n_it == 2 and F(want.score).view(U) == F(s).view(U)
    _bits(want.sequence[0], a)
    pb, pg = _planner(case, monkeypatch, thr=thr, use_graph=True)
    r = pg.plan(pb['state'], seed=SEED, call=CALL)
    assert r[2] == 2
    _same_block(pg.plan_readout(), want, 'the captured plan that stops early')
    pl.close(); pg.close()


@pytest.mark.parametrize('name,use_graph', [('lean_one_quad', True), ('safe', False), ('two_quads', True)])
def test_batch_rows_equal_their_single_plans_and_a_row_that_sat_out_reads_nothing_found(name, use_graph, monkeypatch):
    torch = _torch()
    case = rc.BY_NAME[name]
    pb = rc.problem(case)
    monkeypatch.delenv('CEM_FORCE_ROLLOUT', raising=False)
    _, pcfg = hp.configs(pb, **rc.config_kwargs(case, use_graph=use_graph))
    cap, n = 4, 3
    rng = np.random.default_rng(3)
    states = (pb['state'][None] + rng.normal(0, 0.05, (cap, case.obs))).astype(F)
    calls = np.array([CALL, CALL + 7, (2 << 32) + 1, CALL + 9], np.uint64)
    bp = BatchCemPlanner(pcfg, cap)
    bp.set_weights(pb['weights']); bp.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    bp.set_plan_readout(True)
    bp.plan_batch(states, seed=SEED, calls=calls)                                 # all four rows live: row 3 finds something
    assert bp.plan_readout(cap - 1).candidate >= 0
    for rep in range(2):
        acts, scores, iters = bp.plan_batch(states[:n], seed=SEED, calls=calls[:n])
    for b in range(n):
        _, pl = _planner(case, monkeypatch)
        a, s, it = pl.plan(states[b], seed=SEED, call=int(calls[b]))
        want = pl.plan_readout()
        pl.close()
        _bits(acts[b], a, 'problem %d: action' % b)
        got = bp.plan_readout(b)
        _same_block(got, want, 'problem %d' % b)
        _bits(got.sequence[0], acts[b]); assert F(got.score).view(U) == F(scores[b]).view(U)
    _same_block(bp.plan_readout(cap - 1), rc.empty(case), 'the row that sat the plan out')
    assert _status(bp.plan_readout, cap) == INVALID_ARG and _status(bp.plan_readout, -1) == INVALID_ARG
    torch.cuda.synchronize()
    bp.close()


# ------------------------------------------------------------------------------------------------- 4: the oracle
def _check_against_oracle(case, got, block, trace, what):
    assert (got.candidate, got.iteration, got.flags) == (block.candidate, block.iteration, 0), (what, got, block)
    _bits(got.sequence, block.sequence, '%s: sequence' % what)
    err = np.abs(got.particle_returns.astype(np.float64) - block.particle_returns.astype(np.float64))
    bar = rc.SCORE_BAR + 6e-8 * np.abs(block.particle_returns)                    # 5e-6 + half an ulp
    print('%s: max particle-return error %.3g (bar %.3g), score error %.3g' % (what, err.max(), bar.min(), abs(float(got.score) - float(block.score))))
    assert (err <= bar).all(), (what, err, bar)
    np.testing.assert_array_equal(got.cost_counts, block.cost_counts, err_msg='%s: cost_counts' % what)


@pytest.mark.parametrize('case,seed', rc.ORACLE_CASES, ids=['%s_seed%d' % (c.name, s) for c, s in rc.ORACLE_CASES])
def test_whole_plan_against_the_oracle(case, seed, monkeypatch):
    """sample -> scores -> select and refit -> track replayed by the fp32 oracle on the same noise tensors.  The seeds keep the winner
    more than rc.ORACLE_GAP clear of the runner-up and of the best-so-far score (tests/test_readout_cases_cpu.py): candidate and
    iteration must be EQUAL, the sequence bit-exact, the returns within the per-candidate score bar, the cost counts exact."""
    pb, pl = _planner(case, monkeypatch)
    ra, rs, rit, trace, block = rc.oracle_plan(case, seed)
    ea, em, eo = hp.noise(I, case.N, case.H, case.act, case.P, case.obs, seed=seed)
    a, s, n_it = pl.plan(pb['state'], eps_act=ea, eps_model=em, eps_out=eo)
    assert n_it == rit == I
    _check_against_oracle(case, pl.plan_readout(), block, trace, '%s seed %d' % (case.name, seed))
    pl.close()


def test_a_philox_plan_replayed_by_the_oracle_on_the_filled_noise(monkeypatch):
    """The plan draws its own noise (the lean kernels), cem_fill_noise hands the oracle the same streams."""
    from oracle import cem_oracle as oc
    case = rc.BY_NAME['lean_one_quad']
    pb, pl = _planner(case, monkeypatch)
    assert pl.rollout_path() == 'lean'
    ea, em, eo = (_np(t) for t in pl.fill_noise(seed=SEED, call=CALL))
    a, s, n_it = pl.plan(pb['state'], seed=SEED, call=CALL)
    got = pl.plan_readout()
    ocfg, _ = hp.configs(pb, **rc.config_kwargs(case))
    lb, ub, mu0, sg0 = oc.sampling_params(pb['low'], pb['high'])
    mu = np.broadcast_to(mu0, (case.H, case.act)).astype(F).copy()
    sigma = np.broadcast_to(sg0, (case.H, case.act)).astype(F).copy()
    best, best_score, block, trace = np.zeros(case.act, F), F(-np.inf), rc.empty(case), []
    for it in range(I):
        actions = oc.sample_actions(mu, sigma, lb, ub, ea[it])
        scores, traj = oc.candidate_scores(pb['state'], actions, pb['weights'], pb['inputs_min'], pb['inputs_max'], em[it], ocfg, pb['scorer'],
                                           return_traj=True)
        ret, _ = rc.oracle_evidence(traj, case.P, case.N, pb['scorer'], case.variant)
        before = best_score
        mu, sigma, best, best_score, elite, stop = oc.select_and_refit(scores, actions, mu, sigma, best, best_score, ocfg)
        block = track_best(block, it, it + 1, best_score, scores, elite, actions, ret, None, n=case.N)
        trace.append(dict(scores=scores, before=before))
    margins = rc.oracle_margins(trace)
    print('margins', margins)
    assert min(min(m) for m in margins) > rc.ORACLE_GAP, 'this (seed, call) puts the oracle\'s winner within the bar of its runner-up: %r' % (margins,)
    _check_against_oracle(case, got, block, trace, 'philox plan')
    pl.close()


# ------------------------------------------------------------------------------------------------- 5: off is off
def test_off_is_off(monkeypatch):
    case = rc.BY_NAME['lean_one_quad']
    pb, fresh = _planner(case, monkeypatch, on=False, use_graph=True)
    pb, pl = _planner(case, monkeypatch, on=False, use_graph=True)
    base = fresh.launches_per_iteration()
    assert base == 2 and pl.rollout_path() == 'lean'                              # the rollout (which samples) and the select (which reduces)
    assert _status(pl.plan_readout) == STATE                                      # never enabled: no allocation, nothing to read
    want = fresh.plan(pb['state'], seed=SEED, call=CALL)
    assert fresh.graph_status() == 'graph'
    torch = _torch()
    nodes_off = _graph_nodes(fresh)
    pl.set_plan_readout(True)
    assert pl.launches_per_iteration() == base + 1 and pl.rollout_path() == 'lean' and pl.rollout_form(0) == fresh.rollout_form(0)
    got = pl.plan(pb['state'], seed=SEED, call=CALL)
    assert pl.graph_status() == 'graph' and _graph_nodes(pl) == nodes_off + I     # one tracker per iteration
    _bits(got[0], want[0], 'on: action'); assert F(got[1]).view(U) == F(want[1]).view(U) and got[2] == want[2]
    assert pl.plan_readout().candidate >= 0
    pl.set_plan_readout(False)
    assert not pl.plan_readout_enabled() and pl.launches_per_iteration() == base and _status(pl.plan_readout) == STATE
    got = pl.plan(pb['state'], seed=SEED, call=CALL)
    assert pl.graph_status() == 'graph' and _graph_nodes(pl) == nodes_off
    _bits(got[0], want[0], 'off again: action'); assert F(got[1]).view(U) == F(want[1]).view(U) and got[2] == want[2]
    for key in ('mu_sigma', 'elite_idx', 'actions'):
        _bits(_np(getattr(pl, key)()), _np(getattr(fresh, key)()), key)
    torch.cuda.synchronize()
    fresh.close(); pl.close()


def test_a_timing_handle_books_the_tracker_with_the_select(monkeypatch):
    case = rc.BY_NAME['lean_one_quad']
    pb, off = _planner(case, monkeypatch, on=False)
    pb, pl = _planner(case, monkeypatch)
    want = off.plan(pb['state'], seed=SEED, call=CALL)
    plain = pl.plan(pb['state'], seed=SEED, call=CALL)
    block = pl.plan_readout()
    for p in (off, pl):
        p.set_timing(True)
    off.plan(pb['state'], seed=SEED, call=CALL)
    got = pl.plan(pb['state'], seed=SEED, call=CALL)
    t_off, t_on = off.last_timing(), pl.last_timing()
    for r in (plain, got):
        _bits(r[0], want[0], 'action'); assert F(r[1]).view(U) == F(want[1]).view(U) and r[2] == want[2]
    _same_block(pl.plan_readout(), block, 'the timed plan')
    # the same launches are timed as rollouts on both handles; the tracker's time is inside the select's, which stays a positive number
    assert t_on['rollout_launches'] == t_off['rollout_launches'] > 0 and t_on['select_ms'] > 0 and t_off['select_ms'] > 0
    for key in ('reduce_ms', 'sampler_ms'):                                       # (booked nowhere else: what is folded on one handle is on the other)
        assert (t_on[key] == 0.0) == (t_off[key] == 0.0), (key, t_on, t_off)
    off.close(); pl.close()


def _graph_nodes(pl):
    """Nodes of the handle's captured plan, as the runtime counts them."""
    n = pl.graph_nodes()
    assert n > 0
    return n


# ------------------------------------------------------------------------------------------------- 6: together with the other settings
def _combined(name):
    lean, safe = rc.BY_NAME['lean_one_quad'], rc.BY_NAME['safe']
    if name == 'keep_elites':
        return lean, lambda pl: pl.set_elite_carry(3)
    if name == 'mean_candidate':
        return lean, lambda pl: pl.set_mean_candidate(True)
    if name == 'elite_temperature':
        return lean, lambda pl: pl.set_refit('softmax', 0.5)
    if name == 'noise_beta':
        return lean, lambda pl: pl.set_action_noise('powerlaw', 1.0)
    if name == 'warm_start':
        def warm(pl):
            pl.set_warm_start(shift=1, tail='box', sigma='keep', floor_frac=0.25)
            pl.set_init_mode('shift')
        return lean, warm
    if name == 'risk_level':
        return lean, lambda pl: pl.set_particle_objective('lower_tail', 2)
    if name == 'cost_budget':
        def budget(pl):
            pl.set_constraint('budget', 0)
            pl.set_cost_budget(0.5)
        return safe, budget
    raise KeyError(name)


@pytest.mark.parametrize('name', ['keep_elites', 'mean_candidate', 'elite_temperature', 'noise_beta', 'warm_start', 'risk_level', 'cost_budget'])
def test_together_with_the_other_settings(name, monkeypatch):
    """Two plans in a row (the second warm, where that applies): stepwise launch by launch against track_best, the plan's invariants,
    and the captured plan leaves the same block.  Beyond the tracker, what this compares is the library with itself: a mistake in the
    host path the plan forms share is held by tests/test_gpu_option_fuzz.py, which checks option combinations stage by stage against the
    composed restatement of tests/composed_cases.py."""
    case, setup = _combined(name)
    pb, ps = _planner(case, monkeypatch)
    pb, pg = _planner(case, monkeypatch, use_graph=True)
    for pl in (ps, pg):
        setup(pl)
        assert pl.plan_readout_enabled()                                          # the other setters leave it on
    for j in range(2):
        ps.plan_begin(pb['state'], seed=SEED, call=CALL + j)
        block = ps.plan_readout()
        for it in range(I):
            ps.plan_rollout(it)
            acts = _np(ps.actions())
            ps.plan_select(it)
            got = ps.plan_readout()
            block = track_best(block, it, **_launch_inputs(ps, case, it))
            _same_block(got, block, '%s plan %d iteration %d' % (name, j, it))
            if got.iteration == it:
                _bits(got.sequence, acts[got.candidate], 'the sequence is a row of the sample the rollout read')
        a, s, n_it = ps.plan_end()
        final = ps.plan_readout()
        assert final.flags == 0 and final.candidate >= 0
        _bits(final.sequence[0], a, '%s: sequence[0] is the returned action' % name)
        assert F(final.score).view(U) == F(s).view(U)
        r = pg.plan(pb['state'], seed=SEED, call=CALL + j)
        _bits(r[0], a, '%s: graph action' % name)
        _same_block(pg.plan_readout(), final, '%s: graph, plan %d' % (name, j))
        assert pg.graph_status() == 'graph'
    ps.close(); pg.close()


# ------------------------------------------------------------------------------------------------- refusals
def test_refusals(monkeypatch):
    case = rc.BY_NAME['lean_one_quad']
    pb, pl = _planner(case, monkeypatch, on=False)
    lib, h = pl.lib, pl.h
    assert lib.cem_planner_set_plan_readout(h, 2) == INVALID_ARG and lib.cem_planner_set_plan_readout(h, -1) == INVALID_ARG
    assert lib.cem_planner_get_plan_readout(h, None) == INVALID_ARG
    head = _capi.CemPlanReadout()
    assert lib.cem_planner_plan_readout(h, 0, ctypes.byref(head), None, None, None) == STATE       # off
    pl.plan_begin(pb['state'], seed=SEED, call=CALL)
    assert lib.cem_planner_set_plan_readout(h, 1) == STATE and not pl.plan_readout_enabled()
    pl.plan_rollout(0); pl.plan_select(0); pl.plan_end()
    pl.set_plan_readout(True)
    assert lib.cem_planner_plan_readout(h, 0, None, None, None, None) == INVALID_ARG
    assert lib.cem_planner_plan_readout(h, 1, ctypes.byref(head), None, None, None) == INVALID_ARG
    assert lib.cem_planner_plan_readout(h, -1, ctypes.byref(head), None, None, None) == INVALID_ARG
    assert lib.cem_planner_plan_readout(h, 0, ctypes.byref(head), None, None, None) == 0 and head.candidate == -1   # the head alone
    comm_id = ctypes.create_string_buffer(_capi.CEM_COMM_ID_BYTES)
    assert lib.cem_planner_comm_init(h, comm_id, 1, 0) == UNSUPPORTED             # a communicator on an enabled handle
    pl.close()
    for mode in (2, 3):                                                           # outside the one-workgroup select
        pbm, pm = _planner(case, monkeypatch, on=False, select_mode=mode)
        assert _status(pm.set_plan_readout, True) == UNSUPPORTED and _status(pm.set_plan_readout, False) == 0 and not pm.plan_readout_enabled()
        pm.close()
    pbw, pw = _planner(case, monkeypatch, on=False, world_size=2, rank=0)         # sharded: ret is a shard
    assert _status(pw.set_plan_readout, True) == UNSUPPORTED
    pw.close()
    pbp, pp = _planner(case, monkeypatch, on=False, P=rc.MAX_P + 2, E=5, N=10, k=2)    # 130 particles (130 * 10 rows: a multiple of E = 5)
    assert _status(pp.set_plan_readout, True) == UNSUPPORTED
    pp.close()
    pbq = hp.make_problem(case.obs, case.act, 4, case.depth, seed=77, units=case.units)   # ... and 128 are served: the second trip of the ballots
    _, pcfg = hp.configs(pbq, **rc.config_kwargs(case, P=rc.MAX_P, E=4, N=8, k=2, variant='safe'))
    pq = hp.make_planner(pbq, pcfg)
    pq.set_plan_readout(True)
    pq.plan_begin(pbq['state'], seed=SEED, call=CALL)
    pq.plan_rollout(0); pq.plan_select(0)
    got = pq.plan_readout()
    big = rc.Case('p128', case.obs, case.act, case.depth, case.units, 'fp32', 'safe', 8, 4, rc.MAX_P, 2, case.H, 0, 0, False, None, (), ())
    _same_block(got, track_best(rc.empty(big), 0, **_launch_inputs(pq, big, 0)), '128 particles')
    assert got.candidate >= 0
    pq.plan_end()
    pq.close()


# ------------------------------------------------------------------------------------------------- 7: policies
def _obs(scale=1.0):
    st = np.zeros(60, F); st[3:19] = 0.5; st[22:38] = 0.6                          # PointGoal1's goal and hazard lidars (tests/test_gpu_warm_start.py)
    return (st * F(scale)).astype(F)


def _policy(cls_name, seed=11, **kw):
    from tests.test_simba_api import POLICIES_YAML, make_agent_parts, trained_like
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    from ethz_safe_learning_amd.simba.policies.safe_cem_mpc import SafeCemMpc
    name = {'CemMpc': 'cem_mpc', 'SafeCemMpc': 'safe_cem_mpc'}[cls_name]
    env, model, _ = make_agent_parts(name, seed=seed)
    trained_like(model, np.random.default_rng(seed))
    cls = {'CemMpc': CemMpc, 'SafeCemMpc': SafeCemMpc}[cls_name]
    return env, model, cls(model=model, environment=env, **dict(dict(POLICIES_YAML[name], iterations=3), **kw))


@pytest.fixture
def planner_cache_as_found():
    """What these tests add to the shape-keyed handle cache leaves with them, and what they pushed out comes back."""
    from ethz_safe_learning_amd import planner
    before = list(planner._PLANNER_CACHE.items())
    yield
    planner._PLANNER_CACHE.clear()
    planner._PLANNER_CACHE.update(before)


@pytest.mark.parametrize('cls_name,recover', [('CemMpc', None), ('SafeCemMpc', None), ('SafeCemMpc', 1e9), ('SafeCemMpc', -1e9)])
def test_policies_replan_every_two(cls_name, recover, planner_cache_as_found):
    """recover 1e9: every plan falls below it and is replaced by the cost plan, whose sequence must be the one kept; -1e9: none is."""
    _torch()
    kw = dict(replan_every=2, noise_stddev=0.0)
    if recover is not None:
        kw['recover_below'] = recover
    env, model, pol = _policy(cls_name, **kw)
    obs = _obs()
    acts, plans = [], []
    for d in range(4):
        acts.append(pol.generate_action(obs * F(1.0 - 0.01 * d)))
        plans.append(pol.last_plan)
    assert pol._planner.plan_readout_enabled() and pol.planner_config().plan_readout
    assert pol._planner._call == 4                                                # one call number per decision ...
    assert plans[0] is plans[1] and plans[2] is plans[3] and plans[1] is not plans[2]      # ... and one plan per two
    for d in (0, 2):
        _bits(acts[d], plans[d].sequence[0], 'decision %d returns step 0 of its plan' % d)
        _bits(acts[d + 1], plans[d].sequence[1], 'decision %d returns step 1 of the kept sequence' % (d + 1))
        assert plans[d].flags == 0 and plans[d].candidate >= 0
    if recover == 1e9:
        assert pol.last_recovered and pol._cost_planner.plan_readout_enabled()
        _same_block(pol.last_plan, pol._cost_planner.plan_readout(), 'the kept plan is the cost handle\'s')
        assert F(pol.last_plan.score).view(U) == F(pol.last_safety_score).view(U)
    elif recover is not None:
        assert not pol.last_recovered and pol._cost_planner is None
    if recover != 1e9:
        _same_block(pol.last_plan, pol._planner.plan_readout(), 'the kept plan is the planning handle\'s')
        assert F(pol.last_plan.score).view(U) == F(pol.last_score).view(U)
    pol.reset()
    a = pol.generate_action(obs)
    assert pol._planner._call == 5 and pol.last_plan is not plans[3]              # reset() forces a plan
    _bits(a, pol.last_plan.sequence[0])
    seq = pol.generate_action_sequence(obs)
    assert seq.shape == (pol.horizon, 2) and seq.dtype == F
    _bits(seq, pol._cost_planner.plan_readout().sequence if recover == 1e9 else pol._planner.plan_readout().sequence, 'generate_action_sequence is the read-out')
    with pytest.raises(ValueError, match='replan_every'):
        pol.generate_actions(np.stack([obs, obs]))


def test_policy_read_out_with_output_noise_and_batched_rows(planner_cache_as_found):
    _torch()
    env, model, pol = _policy('SafeCemMpc', plan_readout=True, recover_below=-50.0)
    obs = _obs()
    a = pol.generate_action(obs)
    lp = pol.last_plan
    handle = pol._cost_planner if pol.last_recovered else pol._planner
    # the returned action is step 0 plus the output noise of the decision's call number: what a followed decision would add for its own
    _bits(a, lp.sequence[0] + handle.output_noise(pol.seed, 0) * F(pol.noise_stddev), 'action = sequence[0] + noise_stddev * eps_out')
    assert np.isfinite(lp.particle_returns).all() and ((lp.cost_counts >= 0) & (lp.cost_counts <= pol.particles)).all()
    acts = pol.generate_actions(np.stack([obs, _obs(0.9), _obs(0.8)]))
    assert len(pol.last_plans) == 3 and acts.shape == (3, 2)
    for b, lp in enumerate(pol.last_plans):
        assert lp.flags == 0 and lp.candidate >= 0 and lp.sequence.shape == (pol.horizon, 2)
        np.testing.assert_allclose(acts[b], lp.sequence[0], rtol=0, atol=6 * pol.noise_stddev)      # (a normal draw: six sigma)
    env, model, r3 = _policy('CemMpc', replan_every=3, noise_stddev=0.05)
    a0, a1 = r3.generate_action(obs), r3.generate_action(obs)
    _bits(a1, r3.last_plan.sequence[1] + r3._planner.output_noise(r3.seed, 1) * F(0.05), 'a followed decision draws the noise of its own call')
    for bad in (dict(replan_every=0), dict(replan_every=9), dict(replan_every=2, warm_start=True), dict(replan_every=3, keep_elites=0.3, shift_elites=True, warm_shift=2)):
        with pytest.raises(ValueError):
            _policy('CemMpc', **bad)
