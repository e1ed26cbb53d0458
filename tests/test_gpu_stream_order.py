"""The stream-ordering contracts of the Python host layer and the library's own drains, each held with a busy GPU: every handle runs on
a stream of its own, and what keeps results right across those streams is a set of one-line waits, event records and record_stream
calls that no arithmetic test notices the loss of.  Here a producer is made late (A), a consumer early (B, with the handle's stream
busy), a writer follows a reader at once (C), a tensor is dropped while a foreign stream still uses it (D, addresses only) and plans
are issued behind work still on the stream (E).  tests/stream_cases.py is the instrument; every comparison is bit for bit.

Every test first proves that its two streams really run side by side (stream_cases.concurrent) and fails, not skips, when none of
eight fresh streams does."""
import dataclasses
import gc
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

from tests import handover_cases as hc
from tests import helpers as hp
from tests import stream_cases as sc

pytestmark = pytest.mark.gpu

REGIONS = ('wpack', 'bias_h', 'bias_mu', 'bias_var', 'etab')
TR = dict(E=2, D=20, O=17, L=2, units=48, rows=37, batch=16)            # the trainer of its own tests
BIG = 3 * 2 ** 20 + 256                                                 # floats of a block with a segment of its own in torch's allocator (> 10 MiB)


@pytest.fixture(scope='module')
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    sc.calibrate()
    yield torch
    sc.write_report()


def _dev(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _blob(torch, weights):
    from ethz_safe_learning_amd.planner import flatten_weights
    return _dev(torch, flatten_weights(weights))


def _bundle(torch, lean=False, batch=None, **extra):
    """One planner of the generic or the lean shape with everything its tests hand it: true and decoy weights (host and device), states."""
    from ethz_safe_learning_amd import BatchCemPlanner, CemPlanner
    shape, plan = (sc.LEAN, sc.LEAN_PLAN) if lean else (sc.GENERIC, sc.GENERIC_PLAN)
    pb, pb_decoy = hp.make_problem(seed=101, **shape), hp.make_problem(seed=202, **shape)
    _, pcfg = hp.configs(pb, use_graph=lean, **plan)
    pcfg = dataclasses.replace(pcfg, **extra)
    pl = CemPlanner(pcfg) if batch is None else BatchCemPlanner(pcfg, batch)
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    states = np.stack([(pb['state'] + np.float32(0.01 * i)).astype(np.float32) for i in range(3)])
    return types.SimpleNamespace(pb=pb, pcfg=pcfg, pl=pl, state=states[0], states=states, weights=pb['weights'], decoy_weights=pb_decoy['weights'],
                                 w_true=_blob(torch, pb['weights']), w_decoy=_blob(torch, pb_decoy['weights']), **plan)


@pytest.fixture(scope='module')
def _generic(torch):
    b = _bundle(torch)
    yield b
    b.pl.close()


@pytest.fixture
def generic(_generic):
    _generic.pl.set_weights(_generic.weights)                           # (tests leave the decoy or a trainer's weights behind)
    return _generic


@pytest.fixture(scope='module')
def _lean(torch):
    b = _bundle(torch, lean=True)
    b.pl.plan(b.state, seed=1, call=0)                                  # captures the graph: every later plan is a replay with a polled return
    assert b.pl.graph_status() == 'graph' and b.pl.rollout_path() == 'lean'
    yield b
    b.pl.close()


@pytest.fixture
def lean(_lean):
    _lean.pl.set_weights(_lean.weights)
    return _lean


@pytest.fixture(scope='module')
def _batch(torch):
    b = _bundle(torch, batch=3)
    yield b
    b.pl.close()


@pytest.fixture
def batch(_batch):
    _batch.pl.set_weights(_batch.weights)
    return _batch


def _noise(torch, b, seed, lead=()):
    rng = np.random.default_rng(seed)
    O, A = b.pcfg.obs_dim, b.pcfg.act_dim
    return (_dev(torch, rng.standard_normal(lead + (b.I, b.N, b.H, A)).astype(np.float32)),
            _dev(torch, rng.standard_normal(lead + (b.I, b.H, b.P * b.N, O)).astype(np.float32)))


# =====================================================================================================================================
# (A) inputs produced late on torch's current stream
# =====================================================================================================================================
@pytest.mark.parametrize('shape', ['eager', 'graph'])
def test_set_weights_dev_waits_for_a_late_blob(torch, generic, lean, shape):
    """planner.py:465 (set_weights_dev -> _wait_inputs, planner.py:389): the pack kernels wait for the blob; the plan behind them — eager,
    and replayed through the captured graph — is the true weights' plan."""
    b = generic if shape == 'eager' else lean
    buf = torch.empty_like(b.w_true)

    def call():
        b.pl.set_weights_dev(buf)
        return b.pl.plan(b.state, seed=3, call=7)
    sc.check_late_input(b.pl.stream, buf, b.w_true, b.w_decoy, call, 'set_weights_dev+plan[%s]' % shape)
    assert b.pl.graph_status() == ('eager' if shape == 'eager' else 'graph')


class _FakeEnsemble:
    """What stage_model_weights asks of a model: the weights on the device, and a note of who reads them."""

    def __init__(self, blob):
        self.blob, self.readers = blob, []

    def weights_device(self):
        return self.blob

    def weights_read_on(self, stream):
        self.readers.append(stream)

    def get_weights(self):
        raise AssertionError('stage_model_weights took the host route')


def test_stage_model_weights_waits_for_a_late_blob(torch, generic):
    """planner.py: stage_model_weights -> CemPlanner.set_weights_dev."""
    from ethz_safe_learning_amd.planner import stage_model_weights
    b = generic
    ens = _FakeEnsemble(torch.empty_like(b.w_true))

    def call():
        stage_model_weights(b.pl, ens)
        return b.pl.plan(b.state, seed=3, call=7)
    sc.check_late_input(b.pl.stream, ens.blob, b.w_true, b.w_decoy, call, 'stage_model_weights+plan')
    assert ens.readers and all(s == b.pl.stream for s in ens.readers)   # stage_model_weights: the reader is announced on the planner's stream


def test_batch_set_weights_dev_waits_for_a_late_blob(torch, batch):
    """planner.py:465 on a BatchCemPlanner, then plan_batch (the generator path: no wait of its own)."""
    b = batch
    buf = torch.empty_like(b.w_true)

    def call():
        b.pl.set_weights_dev(buf)
        return b.pl.plan_batch(b.states, seed=3, calls=[4, 5, 6])
    sc.check_late_input(b.pl.stream, buf, b.w_true, b.w_decoy, call, 'batch set_weights_dev+plan_batch')


@pytest.mark.parametrize('which', ['eps_act', 'eps_model'])
@pytest.mark.parametrize('entry', ['plan', 'plan_begin', 'plan_batch'])
def test_plans_wait_for_late_explicit_noise(torch, generic, batch, entry, which):
    """planner.py: CemPlanner.plan, CemPlanner.plan_begin, BatchCemPlanner.plan_batch: explicit noise given as device tensors."""
    b = batch if entry == 'plan_batch' else generic
    lead = (3,) if entry == 'plan_batch' else ()
    true, decoy = _noise(torch, b, 11, lead), _noise(torch, b, 12, lead)
    i = ('eps_act', 'eps_model').index(which)
    buf = torch.empty_like(true[i])
    ea, em = (buf, true[1]) if i == 0 else (true[0], buf)

    def call():
        if entry == 'plan':
            return b.pl.plan(b.state, seed=0, call=0, eps_act=ea, eps_model=em)
        if entry == 'plan_batch':
            return b.pl.plan_batch(b.states, seed=0, calls=[0, 1, 2], eps_act=ea, eps_model=em)
        b.pl.plan_begin(b.state, seed=0, call=0, eps_act=ea, eps_model=em)
        for it in range(b.I):
            b.pl.plan_rollout(it)
            b.pl.plan_select(it)
        return b.pl.plan_end()
    sc.check_late_input(b.pl.stream, buf, true[i], decoy[i], call, '%s[%s]' % (entry, which))


def _model_inputs(torch, b, seed):
    rng = np.random.default_rng(seed)
    O, A, H, n = b.pcfg.obs_dim, b.pcfg.act_dim, b.H, 6
    return dict(s0=_dev(torch, rng.uniform(0.2, 0.9, (n, O)).astype(np.float32)),
                actions=_dev(torch, rng.uniform(-1, 1, (n, H, A)).astype(np.float32)),
                eps_model=_dev(torch, rng.standard_normal((H, n, O)).astype(np.float32)))


@pytest.mark.parametrize('which', ['s0', 'actions', 'eps_model'])
def test_unfold_sequences_waits_for_late_inputs(torch, generic, which):
    """planner.py:909."""
    b = generic
    true, decoy = _model_inputs(torch, b, 21), _model_inputs(torch, b, 22)
    args = dict(true)
    args[which] = torch.empty_like(true[which])
    sc.check_late_input(b.pl.stream, args[which], true[which], decoy[which],
                        lambda: b.pl.unfold_sequences(args['s0'], args['actions'], eps_model=args['eps_model'], return_moments=True),
                        'unfold_sequences[%s]' % which)


def _observations(torch, b, seed, n=9, hot_rows=0):
    """[n, O] lidar-like rows; rows of parity `hot_rows` have a hazard closer than its size (closest distance = lidar_max_dist x the
    smallest bin), so the cost is 1 there and 0 elsewhere."""
    rng = np.random.default_rng(seed)
    obs = rng.uniform(0.2, 0.9, (n, b.pcfg.obs_dim)).astype(np.float32)
    lo, hi, _ = b.pb['scorer'].cost_kinds[0]
    obs[hot_rows::2, lo] = np.float32(0.01)
    return _dev(torch, obs)


def test_compute_objective_waits_for_late_trajectories(torch, generic):
    """planner.py:927."""
    b = generic
    rng = np.random.default_rng(31)
    true, decoy = (_dev(torch, rng.uniform(0.2, 0.9, (b.P * 5, b.H + 1, b.pcfg.obs_dim)).astype(np.float32)) for _ in range(2))
    buf = torch.empty_like(true)
    sc.check_late_input(b.pl.stream, buf, true, decoy, lambda: b.pl.compute_objective(buf), 'compute_objective')


@pytest.mark.parametrize('which', ['observations', 'next_observations'])
def test_scorer_reward_waits_for_late_observations(torch, generic, which):
    """planner.py:940."""
    b = generic
    true, decoy, other = (_observations(torch, b, s) for s in (41, 42, 43))
    buf = torch.empty_like(true)
    args = (buf, other) if which == 'observations' else (other, buf)
    sc.check_late_input(b.pl.stream, buf, true, decoy, lambda: b.pl.scorer_reward(*args), 'scorer_reward[%s]' % which)


def test_scorer_cost_waits_for_late_observations(torch, generic):
    """planner.py:951."""
    b = generic
    true, decoy = _observations(torch, b, 44, hot_rows=0), _observations(torch, b, 45, hot_rows=1)
    buf = torch.empty_like(true)
    sc.check_late_input(b.pl.stream, buf, true, decoy, lambda: b.pl.scorer_cost(buf), 'scorer_cost')


def _trainer_shape(D, units, E=2, O=17, L=2):
    return types.SimpleNamespace(obs_dim=O, act_dim=D - O, units=units, n_layers=L, ensemble_size=E)


def _trainer(D=TR['D'], units=TR['units']):
    from ethz_safe_learning_amd.trainer import CemTrainer
    tr = CemTrainer(D, TR['O'], units, TR['L'], TR['E'], batch_size=TR['batch'])
    w0 = hc.weights(_trainer_shape(D, units), seed=51)
    tr.set_state(w0)
    return tr, w0


def _training_data(torch, D, seed):
    rng = np.random.default_rng(seed)
    n, E = TR['rows'], TR['E']
    return dict(x=_dev(torch, rng.normal(0, 1, (n, D)).astype(np.float32)), y=_dev(torch, rng.normal(0, 1, (n, TR['O'])).astype(np.float32)),
                perm=_dev(torch, np.stack([rng.permutation(n) for _ in range(E)]).astype(np.int32)))


@pytest.fixture(scope='module')
def trainer(torch):
    tr, w0 = _trainer()
    yield types.SimpleNamespace(tr=tr, w0=w0)
    tr.close()


@pytest.mark.parametrize('entry,which', [(e, w) for e in ('step', 'steps', 'validation_loss') for w in ('x', 'y', 'perm')
                                         if (e, w) != ('validation_loss', 'perm')])
def test_trainer_waits_for_late_training_data(torch, trainer, entry, which):
    """trainer.py:109 (step), trainer.py:124 (steps), trainer.py:131 (validation_loss; it takes no permutation: x and y only)."""
    tr = trainer.tr
    true, decoy = _training_data(torch, TR['D'], 61), _training_data(torch, TR['D'], 62)
    args = dict(true)
    args[which] = torch.empty_like(true[which])
    loss = torch.zeros((2, TR['E']), dtype=torch.float32, device='cuda')

    def prepare():
        tr.set_state(trainer.w0)
        tr.iterations = 0

    def call():
        if entry == 'validation_loss':
            return tr.validation_loss(args['x'], args['y'])
        if entry == 'step':
            tr.step(args['x'], args['y'], args['perm'], 3, 16, 1e-2, loss[0])
        else:
            tr.steps(args['x'], args['y'], args['perm'], [0, 16], [16, 16], [1e-2, 1e-2], loss)
        tr.synchronize()
        return tr.weights_dev().clone(), loss.clone()
    sc.check_late_input(tr.stream, args[which], true[which], decoy[which], call, 'trainer.%s[%s]' % (entry, which), prepare=prepare)


@pytest.mark.parametrize('which', ['x', 'eps'])
@pytest.mark.parametrize('map', ['split', 'all'])
def test_forward_waits_for_late_inputs(torch, trainer, map, which):
    """trainer.py:164."""
    tr = trainer.tr
    tr.set_state(trainer.w0)
    n = TR['rows'] - (TR['rows'] % TR['E'] if map == 'split' else 0)
    shape = (n, TR['O']) if map == 'split' else (TR['E'], n, TR['O'])
    rng = np.random.default_rng(71)
    xs = [_dev(torch, rng.normal(0, 1, (n, TR['D'])).astype(np.float32)) for _ in range(2)]
    es = [_dev(torch, rng.standard_normal(shape).astype(np.float32)) for _ in range(2)]
    true, decoy = (xs if which == 'x' else es)
    buf = torch.empty_like(true)
    x, eps = (buf, es[0]) if which == 'x' else (xs[0], buf)
    sc.check_late_input(tr.stream, buf, true, decoy, lambda: tr.forward(x, map=map, eps=eps, want=('mu', 'var', 'sd', 'sample')),
                        'forward[%s,%s]' % (map, which))


# =====================================================================================================================================
# (B) outputs consumed early: the handle's stream is busy when the call is made
# =====================================================================================================================================
F32, I32, U8 = 'float32', 'int32', 'uint8'


def _specs(torch, *specs):
    return [(shape, getattr(torch, dt)) for shape, dt in specs]


@pytest.mark.parametrize('moments', [False, True])
def test_unfold_sequences_returns_finished_tensors(torch, generic, moments):
    """cem_capi.hip: the drain at the end of cem_unfold_sequences."""
    b = generic
    a = _model_inputs(torch, b, 23)
    O, H = b.pcfg.obs_dim, b.H
    sc.check_early_output(b.pl.stream, lambda: b.pl.unfold_sequences(a['s0'], a['actions'], eps_model=a['eps_model'], return_moments=moments),
                          'unfold_sequences[moments=%s]' % moments,
                          _specs(torch, ((6, H + 1, O), F32), *([((6, H, O), F32)] * 2 if moments else [])))


def test_compute_objective_returns_finished_scores(torch, generic):
    """cem_capi.hip: cem_compute_objective."""
    b = generic
    traj = _dev(torch, np.random.default_rng(32).uniform(0.2, 0.9, (b.P * 5, b.H + 1, b.pcfg.obs_dim)).astype(np.float32))
    sc.check_early_output(b.pl.stream, lambda: b.pl.compute_objective(traj), 'compute_objective', _specs(torch, ((5,), F32)))


def test_scorer_ops_return_finished_tensors(torch, generic):
    """cem_capi.hip: scorer_op, behind cem_scorer_reward and cem_scorer_cost."""
    b = generic
    obs, nxt = _observations(torch, b, 46), _observations(torch, b, 47)
    sc.check_early_output(b.pl.stream, lambda: b.pl.scorer_reward(obs, nxt), 'scorer_reward', _specs(torch, ((9,), F32), ((9,), U8)))
    sc.check_early_output(b.pl.stream, lambda: b.pl.scorer_cost(obs), 'scorer_cost', _specs(torch, ((9,), F32)))


def test_noise_ops_return_finished_tensors(torch, generic):
    """cem_capi.hip: cem_fill_noise (behind fill_noise and output_noise) and cem_philox_words."""
    b = generic
    c = b.pcfg
    sc.check_early_output(b.pl.stream, lambda: b.pl.fill_noise(seed=5, call=6), 'fill_noise',
                          _specs(torch, ((b.I, b.N, b.H, c.act_dim), F32), ((b.I, b.H, b.P * b.N, c.obs_dim), F32), ((c.act_dim,), F32)))
    sc.check_early_output(b.pl.stream, lambda: b.pl.output_noise(seed=5, call=6), 'output_noise', _specs(torch, ((c.act_dim,), F32)))
    sc.check_early_output(b.pl.stream, lambda: b.pl.philox_words(5, 6, 1, 0, 2, 0, 3, 40), 'philox_words', _specs(torch, ((40, 4), I32)))


@pytest.mark.parametrize('map', ['split', 'all'])
def test_forward_outputs_are_ordered_behind_the_trainer(torch, trainer, map):
    """trainer.py:171 (cur.wait_stream(self.stream)): all four outputs, both maps."""
    tr = trainer.tr
    tr.set_state(trainer.w0)
    n = TR['rows'] - (TR['rows'] % TR['E'] if map == 'split' else 0)
    shape = (n, TR['O']) if map == 'split' else (TR['E'], n, TR['O'])
    x = _dev(torch, np.random.default_rng(72).normal(0, 1, (n, TR['D'])).astype(np.float32))
    sc.check_early_output(tr.stream, lambda: tr.forward(x, map=map, seed=3, call=4, want=('mu', 'var', 'sd', 'sample')), 'forward[%s]' % map,
                          _specs(torch, *([(shape, F32)] * 4)))


def _ensemble(D, units, **kw):
    from ethz_safe_learning_amd.simba.models.mlp_ensemble import MlpEnsemble
    args = dict(batch_size=TR['batch'], validation_split=0.0, training_steps=7, learning_rate=1e-2,
                mlp_params=dict(n_layers=TR['L'], units=units, activation='tf.nn.relu', dropout_rate=0.0), seed=5)
    args.update(kw)
    return MlpEnsemble(D, TR['O'], TR['E'], **args)


def test_ensemble_forward_and_call_with_device_inputs(torch):
    """trainer.py:171 through MlpEnsemble.forward and __call__ (mlp_ensemble.py:136): device inputs give device outputs, finished."""
    ens = _ensemble(TR['D'], TR['units'])
    tr = ens._get_trainer()
    x = _dev(torch, np.random.default_rng(73).normal(0, 1, (36, TR['D'])).astype(np.float32))
    sc.check_early_output(tr.stream, lambda: ens.forward(x), 'MlpEnsemble.forward', _specs(torch, *([((36, TR['O']), F32)] * 2)))
    sc.check_early_output(tr.stream, lambda: ens(x, seed=8, call=9), 'MlpEnsemble.__call__', _specs(torch, *([((36, TR['O']), F32)] * 3)))
    tr.close()


ACCESSORS = ('actions', 'scores_local', 'mu_sigma', 'elite_idx', 'returns', 'costs', 'result_block')


@pytest.mark.parametrize('name', ACCESSORS)
def test_accessors_drain_the_stream_behind_a_polled_plan(torch, lean, name):
    """planner.py:409 (_view, sync=True; the comment at planner.py:399): plan() on a captured graph returns on the polled result block, not
    on a drained stream.  The kernels that may still run behind that result are stood in for by a busy kernel and a copy queued on the
    planner's stream: the accessor's tensor, copied at once on another stream, holds what that copy wrote."""
    pl = lean.pl
    side = sc.consumer_for(pl.stream, 'accessor ' + name)
    with torch.cuda.stream(side):
        pl.plan(lean.state, seed=2, call=3)
        raw = getattr(pl, name)(sync=False).reshape(-1).view(torch.uint8)
        pl.synchronize()
        before = raw.clone()
        marker = before.bitwise_xor(0x55)
        torch.cuda.synchronize()
        pl.plan(lean.state, seed=2, call=4)                             # the polled return: the stream may still be draining here
        sc.delay(pl.stream, sc.MIN_MS, 'accessor ' + name)
        with torch.cuda.stream(pl.stream):
            raw.copy_(marker)
        got = getattr(pl, name)().clone()
        torch.cuda.synchronize()
        assert not sc.same(sc.bits(marker), sc.bits(before))
        sc.assert_same(sc.bits(got), sc.bits(marker), name)


def test_carry_drains_the_stream(torch, generic):
    """cem_capi.hip: cem_planner_get_carry: the copies to the host are queued on the planner's stream behind whatever it holds; the
    call returns only once they have landed."""
    pl = generic.pl
    pl.plan(generic.state, seed=2, call=3)
    mu, sigma, valid = pl.carry()
    assert valid
    ms = pl.mu_sigma(sync=False)
    np.testing.assert_array_equal(ms.cpu().numpy(), np.stack([mu, sigma]))       # the carry still lives in the plan's mu / sigma slice
    marker = (ms * 2 + 1).clone()
    torch.cuda.synchronize()
    sc.delay(pl.stream, sc.MIN_MS, 'carry')
    with torch.cuda.stream(pl.stream):
        ms.copy_(marker)
    mu2, sigma2, _ = pl.carry()
    np.testing.assert_array_equal(np.stack([mu2, sigma2]), marker.cpu().numpy())


def _first_iteration(pl, state, call):
    pl.plan_begin(state, seed=4, call=call)
    pl.plan_rollout(0)
    pl.plan_select(0)


def _rest_of_plan(pl, I):
    for it in range(1, I):
        pl.plan_rollout(it)
        pl.plan_select(it)
    return pl.plan_end()


DRAINED = {
    # name: (PlannerConfig overrides, what to do after create, the read)
    'plan_readout': (dict(plan_readout=True), None, lambda pl: tuple(pl.plan_readout())),
    'elite_store': (dict(keep_elites=2), None, lambda pl: pl.elite_store()),
    'refit_stats': (dict(refit='softmax', refit_temperature=1.0), None, lambda pl: pl.refit_stats(n=1)),
    'constraint_costs': (dict(variant='safe', constraint='budget'), lambda pl: pl.set_cost_budget(1.0), lambda pl: pl.constraint_costs()),
}


@pytest.mark.parametrize('name', sorted(DRAINED))
def test_host_reads_drain_the_stream(torch, name):
    """cem_capi.hip: cem_planner_plan_readout, cem_planner_elite_store, cem_planner_refit_stats and
    cem_planner_constraint_costs: each copies from an allocation of the library's with a blocking copy that knows nothing of the
    planner's stream, so each drains that stream first.  A stepwise plan's first iteration is queued behind a busy kernel; the read
    returns that iteration's values, not the previous plan's."""
    extra, after, read = DRAINED[name]
    null = torch.cuda.default_stream()

    def make():
        b = _bundle(torch, **extra)
        if after:
            after(b.pl)
        b.close = b.pl.close
        return b
    b = sc.handle_beside(make, lambda h: sc.concurrent(h.pl.stream, null), name)
    pl, A, B = b.pl, (b.states[1], 12), (b.states[0], 11)              # (state, call): two plans with nothing in common
    refs = []
    for plan in (A, B, A):                                              # (the first: warm-up, so that the timed one launches nothing for the first time)
        torch.cuda.synchronize()
        ms, _ = sc.event_ms(pl.stream, lambda: _first_iteration(pl, *plan))
        refs.append(sc.bits(read(pl)))
        _rest_of_plan(pl, b.I)
        if plan is B:
            d = sc.delay_ms(ms)
            sc.log('delay %s: the first iteration takes %.3f ms on the idle handle -> %.1f ms' % (name, ms, d))
    assert not sc.same(refs[1], refs[2]), name
    torch.cuda.synchronize()                                            # what the allocations hold now: the whole of plan A
    sc.delay(pl.stream, d)
    _first_iteration(pl, *B)
    got = sc.bits(read(pl))
    _rest_of_plan(pl, b.I)
    sc.assert_same(got, refs[1], name)
    pl.close()


# =====================================================================================================================================
# (C) write after read on the trainer's blob
# =====================================================================================================================================
def _images_of(H, weights):
    H.set_weights(weights)
    return H.weight_images()


def _assert_images(got, want, other, what):
    assert any(not np.array_equal(want[k], other[k]) for k in REGIONS), '%s: the step left the images as they were' % what
    for k in REGIONS:
        np.testing.assert_array_equal(got[k], want[k], err_msg='%s %s' % (what, k))


def _planner_like(b):
    from ethz_safe_learning_amd import CemPlanner
    pl = CemPlanner(b.pcfg)
    pl.set_normaliser(b.pb['inputs_min'], b.pb['inputs_max'])
    return pl


def test_set_weights_from_holds_the_trainer_back_until_the_images_are_packed(torch, generic):
    """planner.py:487-488 (set_weights_from: the event recorded on the planner's stream behind the pack kernels, and the trainer's wait on
    it).  Reading orders the pack kernels behind the trainer; this orders the trainer's NEXT write behind the pack kernels.  With the
    planner's stream busy, a step issued right after the hand-over must not reach the blob before the pack kernels have read it: the
    images are those of the weights before the step, as a second handle fed over the host has them."""
    D = generic.pcfg.obs_dim + generic.pcfg.act_dim
    tr, w0 = _trainer(D, generic.pcfg.units)
    data = _training_data(torch, D, 81)
    loss = torch.zeros(TR['E'], dtype=torch.float32, device='cuda')
    pl = sc.handle_beside(lambda: _planner_like(generic), lambda h: sc.concurrent(h.stream, tr.stream), 'set_weights_from (write after read)')
    before = _images_of(generic.pl, w0)
    with torch.cuda.stream(torch.cuda.Stream()):
        ms, _ = sc.event_ms(pl.stream, lambda: pl.set_weights_from(tr))
        d = sc.delay_ms(ms)
        sc.log('delay set_weights_from: the hand-over takes %.3f ms on the idle handle -> %.1f ms' % (ms, d))
        sc.delay(pl.stream, d)
        pl.set_weights_from(tr)
        tr.step(data['x'], data['y'], data['perm'], 0, 16, 1e-2, loss)
        torch.cuda.synchronize()
    got = pl.weight_images()
    _assert_images(got, before, _images_of(generic.pl, tr.get_weights()), 'set_weights_from, then step')
    pl.close(); tr.close()


def test_set_weights_from_takes_the_weights_behind_a_late_step(torch, generic):
    """planner.py:482-483 (ev.record(trainer.stream) / self.stream.wait_event(ev)): the converse — the trainer's stream is busy in front of
    a step, the hand-over follows at once, and the planner gets the weights after the step."""
    D = generic.pcfg.obs_dim + generic.pcfg.act_dim
    tr, w0 = _trainer(D, generic.pcfg.units)
    data = _training_data(torch, D, 82)
    loss = torch.zeros(TR['E'], dtype=torch.float32, device='cuda')
    pl = sc.handle_beside(lambda: _planner_like(generic), lambda h: sc.concurrent(tr.stream, h.stream), 'set_weights_from (read after write)')
    before = _images_of(generic.pl, w0)
    with torch.cuda.stream(torch.cuda.Stream()):
        ms, _ = sc.event_ms(tr.stream, lambda: tr.step(data['x'], data['y'], data['perm'], 0, 16, 1e-2, loss))
        d = sc.delay_ms(ms)
        sc.log('delay step: a step takes %.3f ms on the idle trainer -> %.1f ms' % (ms, d))
        tr.set_state(w0)
        tr.iterations = 0
        sc.delay(tr.stream, d)
        tr.step(data['x'], data['y'], data['perm'], 0, 16, 1e-2, loss)
        pl.set_weights_from(tr)
        torch.cuda.synchronize()
    got = pl.weight_images()
    _assert_images(got, _images_of(generic.pl, tr.get_weights()), before, 'step, then set_weights_from')
    pl.close(); tr.close()


@pytest.mark.parametrize('writer', ['forward_after_set_weights', 'fit'])
def test_ensemble_holds_its_trainer_back_behind_a_staging_planner(torch, generic, writer):
    """planner.py: stage_model_weights -> weights_read_on, mlp_ensemble.py:118 (the event recorded on the reader's stream) and
    mlp_ensemble.py:96-97 (_get_trainer: the trainer's stream waits for every reader).  The planner's stream is busy when it stages the
    model's device weights; the model's next write of the blob — a forward that re-stages weights replaced from outside, or a fit —
    follows at once and must not reach the blob before the pack kernels have read it."""
    from ethz_safe_learning_amd.planner import stage_model_weights
    D = generic.pcfg.obs_dim + generic.pcfg.act_dim
    shape = _trainer_shape(D, generic.pcfg.units)
    w0, w1 = hc.weights(shape, seed=91), hc.weights(shape, seed=92)
    ens = _ensemble(D, generic.pcfg.units, training_steps=2)
    ens.set_weights(w0)
    tr = ens._get_trainer()
    assert ens.weights_device() is not None
    rng = np.random.default_rng(93)
    x = rng.normal(0, 1, (TR['rows'], D)).astype(np.float32)
    y = rng.normal(0, 1, (TR['rows'], TR['O'])).astype(np.float32)
    pl = sc.handle_beside(lambda: _planner_like(generic), lambda h: sc.concurrent(h.stream, tr.stream), 'stage_model_weights, then ' + writer)
    before = _images_of(generic.pl, w0)
    with torch.cuda.stream(torch.cuda.Stream()):
        ms, _ = sc.event_ms(pl.stream, lambda: stage_model_weights(pl, ens))
        d = sc.delay_ms(ms)
        sc.log('delay stage_model_weights: staging takes %.3f ms on the idle handle -> %.1f ms' % (ms, d))
        sc.delay(pl.stream, d)
        stage_model_weights(pl, ens)
        assert pl.have_device_weights
        if writer == 'fit':
            np.random.seed(3)
            ens.fit(x, y)
        else:
            ens.set_weights(w1)
            ens.forward(_dev(torch, x[:36]))
        torch.cuda.synchronize()
    got = pl.weight_images()
    _assert_images(got, before, _images_of(generic.pl, ens.get_weights()), 'stage_model_weights, then ' + writer)
    pl.close(); tr.close()


# =====================================================================================================================================
# (D) lifetime: record_stream (addresses only: nothing here touches memory that has gone back to the allocator)
# =====================================================================================================================================
def _big(torch):
    return torch.empty(BIG, dtype=torch.float32, device='cuda')


def test_set_weights_dev_keeps_the_blob_from_the_allocator(torch, generic):
    """planner.py:467 (blob.record_stream(self.stream)): a blob dropped right after the hand-over, while the planner's stream has not
    run the pack kernels yet, does not come back from the allocator; a block freed without any foreign-stream use does (the control)."""
    pl, n = generic.pl, generic.w_true.numel()
    with torch.cuda.stream(torch.cuda.Stream()):
        gc.collect()
        t = _big(torch)
        p_control = t.data_ptr()
        del t
        block = _big(torch)
        p = block.data_ptr()
        assert p == p_control                                           # control: the allocator hands a freed block of this size out again
        blob = block[:n]
        blob.copy_(generic.w_true)
        torch.cuda.synchronize()
        sc.delay(pl.stream, sc.MIN_MS, 'lifetime set_weights_dev')
        pl.set_weights_dev(blob)
        del blob, block
        t = _big(torch)
        assert t.data_ptr() != p                                        # the pack kernels are still pending
        pl.synchronize()
        del t
        t = _big(torch)                                                 # (it may coincide again now; nothing is asserted)
        sc.log('lifetime set_weights_dev: after synchronize a fresh block is %s the blob\'s' % ('at' if t.data_ptr() == p else 'not at'))


def test_forward_keeps_inputs_and_outputs_from_the_allocator(torch, trainer):
    """trainer.py:168-170 (record_stream on x_dev, eps and every output): all dropped while the trainer's stream has not run the kernel."""
    tr = trainer.tr
    tr.set_state(trainer.w0)
    n, shape = TR['rows'], (TR['E'], TR['rows'], TR['O'])
    want = ('mu', 'var', 'sd', 'sample')
    with torch.cuda.stream(torch.cuda.Stream()):
        gc.collect()
        small = [torch.empty(shape, dtype=torch.float32, device='cuda') for _ in want]
        big = [_big(torch), _big(torch)]
        p_small, p_big = {t.data_ptr() for t in small}, {t.data_ptr() for t in big}
        del small, big
        bx, be = _big(torch), _big(torch)
        small = [torch.empty(shape, dtype=torch.float32, device='cuda') for _ in want]
        assert {bx.data_ptr(), be.data_ptr()} == p_big and {t.data_ptr() for t in small} == p_small      # control
        del small
        x, eps = bx[:n * TR['D']].view(n, TR['D']), be[:int(np.prod(shape))].view(shape)
        x.normal_(); eps.normal_()
        torch.cuda.synchronize()
        sc.delay(tr.stream, sc.MIN_MS, 'lifetime forward')
        outs = tr.forward(x, map='all', eps=eps, want=want)
        p_outs = {t.data_ptr() for t in outs}
        assert p_outs == p_small                                        # (the outputs took the blocks the control freed)
        del x, eps, bx, be, outs
        big = [_big(torch), _big(torch)]
        small = [torch.empty(shape, dtype=torch.float32, device='cuda') for _ in want]
        assert not ({t.data_ptr() for t in big} & p_big)                # x_dev, eps
        assert not ({t.data_ptr() for t in small} & p_outs)             # every output
        tr.synchronize()


def test_fit_records_every_permutation_on_the_trainers_stream(torch, monkeypatch):
    """mlp_ensemble.py:185 (perm_dev.record_stream(tr.stream)): fit runs epochs ahead of the device; every epoch's permutation is known to
    the allocator as in use on the trainer's stream before the first step that reads it is queued, and no two epochs still pending on
    the device share one address.  (fit also keeps the tensors in a list until its final synchronise; the record is what protects them
    should that list ever go.)"""
    from ethz_safe_learning_amd.trainer import CemTrainer
    ens = _ensemble(TR['D'], TR['units'])
    tr = ens._get_trainer()
    recorded, seen = {}, []
    real_record, real_steps = torch.Tensor.record_stream, CemTrainer.steps

    def record_stream(self, stream):
        recorded.setdefault(self.data_ptr(), []).append(stream)
        return real_record(self, stream)

    def steps(self, x_dev, y_dev, perm_dev, *a):
        p = perm_dev.data_ptr()
        if not seen or seen[-1] != p:
            assert p not in seen, 'two epochs pending on the device share a permutation tensor'
            seen.append(p)
        assert any(s == self.stream for s in recorded.get(p, [])), 'steps queued on a permutation the allocator may hand out again'
        return real_steps(self, x_dev, y_dev, perm_dev, *a)
    monkeypatch.setattr(torch.Tensor, 'record_stream', record_stream)
    monkeypatch.setattr(CemTrainer, 'steps', steps)
    rng = np.random.default_rng(95)
    x = rng.normal(0, 1, (TR['rows'], TR['D'])).astype(np.float32)
    np.random.seed(4)
    sc.delay(tr.stream, sc.MIN_MS, 'lifetime fit')                      # the device stays behind the host for the whole fit
    ens.fit(x, rng.normal(0, 1, (TR['rows'], TR['O'])).astype(np.float32))
    assert len(seen) == 3                                               # 7 steps in epochs of 3 batches
    tr.close()


# =====================================================================================================================================
# (E) the polled return
# =====================================================================================================================================
@pytest.mark.parametrize('tail_ms', [30.0, 130.0], ids=['inside_the_poll_window', 'past_the_poll_window'])
def test_plans_issued_behind_pending_work_equal_drained_ones(torch, tail_ms):
    """cem_capi.hip: wait_result and read_results: plan() on a captured graph watches the pinned result block, for up
    to 100 ms, then synchronises the stream.  Two plans are issued back to back, each behind a busy kernel on the planner's stream — the
    second while whatever ran behind the first one's result is still there — and return the action, score and iteration count of the
    same plans on a drained stream."""
    r = sc.polled_pair(tail_ms)
    assert r['ref'][0] != r['ref'][1]
    assert r['got'] == r['ref']


def test_plans_issued_behind_pending_work_without_polling(torch):
    """cem_capi.hip: wait_result (CEM_NO_POLL, read once per process: a child process): the same pair through the stream synchronisation alone."""
    env = dict(os.environ, CEM_NO_POLL='1')
    r = subprocess.run([sys.executable, '-m', 'tests.stream_cases', '30'], env=env, cwd=sc.ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-3000:]
    line = [l for l in r.stdout.splitlines() if l.startswith('POLLED ')][-1]
    child = json.loads(line[len('POLLED '):])
    assert child['got'] == child['ref']
    assert child['ref'] == sc.polled_pair(30.0)['ref']                  # and the child's plans are this process's plans
