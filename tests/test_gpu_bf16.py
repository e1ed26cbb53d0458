"""The reduced-precision rollout (precision 'bf16': csrc/cem_rollout_bf16.h) on the GPU, held to ITS OWN arithmetic — the rounding model
planner.bf16_reference_forward states — at bars worked out from the references alone (tests/bf16_cases.py; tests/test_bf16_cpu.py holds
the fp32-accumulating emulation to the same bars in the kernel's place), and to the invariances that must hold bit for bit within it."""
import numpy as np
import pytest

from ethz_safe_learning_amd import _capi, planner
from ethz_safe_learning_amd.planner import flatten_weights
from oracle import cem_oracle as o
from tests import bf16_cases as bc
from tests import helpers as hp

pytestmark = pytest.mark.gpu
F32 = np.float32


@pytest.fixture(scope='module')
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip('no GPU')
    return torch


def _filled(cls):
    """a handle whose workspace is all 0xFF bytes when the library first sees it (tests/test_gpu_weight_handover.py)"""
    class Filled(cls):
        def _create(self, ws_ptr, nbytes, stream, out):
            self._ws_view.fill_(0xFF)
            self._torch.cuda.synchronize(self.device)
            super()._create(ws_ptr, nbytes, stream, out)
    return Filled


def _device_fed(torch, pb, pcfg):
    from ethz_safe_learning_amd import CemPlanner
    pl = _filled(CemPlanner)(pcfg)
    pl.set_weights_dev(torch.from_numpy(flatten_weights(pb['weights'])).cuda())
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    return pl


# ---- 1. exact cases: layout and packing ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('route', ['host', 'device'])
@pytest.mark.parametrize('dims', bc.SHAPES, ids=bc.SHAPE_IDS)
def test_exact_cases_equal_the_emulation_bit_for_bit(torch, dims, route):
    """Every dense output is one product plus a bias and every float32 sum is exact (bf16_cases.exact_problem), so mu and the
    trajectories equal the emulation with assert_array_equal whatever the summation order; sd within the existing 2e-5.  Through the
    host packer and through the device weight hand-over."""
    O, A, U = dims
    B, H, E = 40, 3, 5
    pb = bc.exact_problem(O, A, U, E=E, seed=O)
    s0, acts, eps = bc.exact_inputs(O, A, B, H, seed=O + 1)
    _, pcfg = hp.configs(pb, N=64, H=4, P=5, E=E, k=6, I=1, precision='bf16')
    pl = hp.make_planner(pb, pcfg) if route == 'host' else _device_fed(torch, pb, pcfg)
    traj, mu, sd = (x.cpu().numpy() for x in pl.unfold_sequences(s0, acts, eps_model=eps, return_moments=True))
    pl.close()
    with bc.emulating(bc.emu64):
        rt, rm, rs = bc.unfold_with_moments(s0, acts, pb['weights'], bc.members_of(B, E), pb['inputs_min'], pb['inputs_max'], eps)
    assert np.abs(rt[:, 1:] - rt[:, :-1]).max() > 0.1 and len(np.unique(planner.rn_bf16(rt) != rt)) == 2       # the states move, and the rounding bites
    np.testing.assert_array_equal(mu, rm)
    np.testing.assert_array_equal(traj, rt)
    np.testing.assert_allclose(sd, rs, rtol=2e-5, atol=2e-5)


# ---- 2. the rounding model on dense random weights ------------------------------------------------------------------------------
@pytest.mark.parametrize('dims', bc.SHAPES, ids=bc.SHAPE_IDS)
def test_trajectories_follow_the_rounding_model(torch, dims):
    """B = 80, H = 8 on make_problem weights and explicit model noise: at every step RMS(kernel - emulation) <= 0.05 x
    RMS(emulation - fp64 oracle) and max |kernel - emulation| <= max |emulation - fp64 oracle| (bf16_cases.RATIO says why 0.05)."""
    pb, s0, acts, eps, emu, ref64 = bc.traj_case(dims)
    _, pcfg = hp.configs(pb, N=64, H=4, P=5, E=5, k=6, I=1, precision='bf16')
    pl = hp.make_planner(pb, pcfg)
    traj = pl.unfold_sequences(s0, acts, eps_model=eps).cpu().numpy()
    pl.close()
    M = [bc.rms(emu[:, t] - ref64[:, t]) for t in range(emu.shape[1])]
    K = [bc.rms(traj[:, t] - emu[:, t]) for t in range(emu.shape[1])]
    print('bf16 obs %d: RMS(emulation - fp64) per step %s | RMS(kernel - emulation) %s | ratios %s' % (
        dims[0], ' '.join('%.2e' % m for m in M[1:]), ' '.join('%.2e' % k for k in K[1:]), ' '.join('%.4f' % (k / m) for k, m in zip(K[1:], M[1:]))))
    bc.check_rounding_model(traj, emu, ref64, 'obs %d' % dims[0])


# ---- 3. scores of one iteration ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['cem', 'safe'])
@pytest.mark.parametrize('rc', [1, 2, 3, 4])
@pytest.mark.parametrize('O,A', [(60, 2), (100, 12)], ids=['obs60', 'obs100'])
def test_scores_follow_the_rounding_model(torch, O, A, rc, variant):
    """N = 256, H = 12, P = E = 5 on explicit noise, every tile size: candidate_scores under the emulation; near-threshold candidates
    (at most 10 %) under the admissible outcomes, the rest under the two conditions of the trajectory test."""
    c = bc.score_case(O, A, variant)
    _, pcfg = hp.configs(c['pb'], variant=variant, post=0.3, precision='bf16', chunks_per_tile=rc, **bc.SCORE_SHAPE)
    pl = hp.make_planner(c['pb'], pcfg)
    pl.plan_begin(c['pb']['state'], eps_act=c['ea'], eps_model=c['em'])
    pl.plan_rollout(0)
    torch.cuda.synchronize()
    sc = pl.scores_local().cpu().numpy().copy()
    pl.plan_end()
    assert pl.tiles()[0] == rc
    pl.close()
    print('bf16 obs %d %s rc %d: %s' % (O, variant, rc, bc.score_figures(sc, c)))
    ratio, near, med, p90 = bc.check_scores(sc, c, 'obs %d %s rc %d' % (O, variant, rc))
    print('bf16 obs %d %s rc %d: score ratio %.4f, %.1f %% near a threshold; flip-free median ratio %.4f, 90th percentile ratio %.4f' % (
        O, variant, rc, ratio, 100 * near, med, p90))


@pytest.mark.parametrize('obs', [60, 84])
@pytest.mark.parametrize('variant', ['cem', 'safe'])
@pytest.mark.parametrize('case', list(hp.SCORER_CASES))
def test_scorer_branches_follow_the_rounding_model(torch, case, variant, obs):
    """Every branch of the scorer (helpers.SCORER_CASES: 0 - 4 constrained kinds, the non-indicator sum, observe_goal_dist, reward clip
    absent / active) in the kernel's own copy of the epilogue, at obs 60 (one input block per wave) and 84 (two), both objectives,
    planning mode on explicit noise at test_rollout_scorer_branches' shape: check_scores against candidate_scores under the emulation,
    and for the safe objective the done-masked per-step cost bytes of every row clear of a threshold, exactly (small integers), against
    the costs on the emulation's trajectory (tests/test_bf16_bars_cpu.py holds the stand-ins and the mutants to the same bars)."""
    c = bc.scorer_case(case, obs, variant)
    n = bc.SCORER_SHAPE
    _, pcfg = hp.configs(c['pb'], variant=variant, post=bc.SCORER_POST, precision='bf16', **n)
    pl = hp.make_planner(c['pb'], pcfg)
    pl.plan_begin(c['pb']['state'], eps_act=c['ea'], eps_model=c['em'])
    pl.plan_rollout(0)
    torch.cuda.synchronize()
    sc = pl.scores_local().cpu().numpy().copy()
    actions = pl.actions().cpu().numpy().copy()
    costs = pl.costs().cpu().numpy().reshape(n['H'], n['P'] * n['N']).astype(np.float64) if variant == 'safe' else None
    pl.plan_end()
    pl.close()
    what = 'bf16 %s obs %d %s' % (case, obs, variant)
    np.testing.assert_array_equal(actions, c['actions'], err_msg=what)
    print('%s: %s' % (what, bc.score_figures(sc, c)))
    ratio, near, med, p90 = bc.check_scores(sc, c, what)
    print('%s: score ratio %.4f, %.1f %% near a threshold; flip-free median ratio %.4f, 90th percentile ratio %.4f' % (what, ratio, 100 * near, med, p90))
    if variant == 'safe':
        np.testing.assert_array_equal(costs[:, c['row_clear']], c['costs'][:, c['row_clear']], err_msg=what)


# ---- 4. bit-identical within the kernel --------------------------------------------------------------------------------------------
def _plan_all(pl, state, seed=9, call=4):
    a, s, it = pl.plan(state, seed=seed, call=call)
    return a, s, it, pl.scores_global().cpu().numpy().copy(), pl.mu_sigma().cpu().numpy().copy()


def _assert_same(x, y):
    for u, v in zip(x, y):
        np.testing.assert_array_equal(np.asarray(v), np.asarray(u))


def test_tile_sizes_ranks_launch_forms_and_weight_routes_are_bit_identical(torch):
    pb = hp.make_problem(60, 2, 5, 4, seed=33)
    N, H, P, E, k, I = 512, 10, 5, 5, 51, 2
    shape = dict(N=N, H=H, P=P, E=E, k=k, I=I, precision='bf16')
    ref = None
    for rc in (0, 1, 2, 3, 4):                                # the automatic size and every explicit one
        _, pcfg = hp.configs(pb, chunks_per_tile=rc, **shape)
        pl = hp.make_planner(pb, pcfg)
        got = _plan_all(pl, pb['state'])
        if ref is None:
            ref = got
            _assert_same(ref, _plan_all(pl, pb['state']))     # two runs of one handle
            assert pl.rollout_path() == 'generic'
        else:
            assert pl.tiles()[0] == rc
            _assert_same(ref, got)
        pl.close()
    # graph against eager (above) against stepwise
    _, pcfg = hp.configs(pb, use_graph=True, **shape)
    pl = hp.make_planner(pb, pcfg)
    _assert_same(ref, _plan_all(pl, pb['state']))
    _assert_same(ref, _plan_all(pl, pb['state']))             # the replay
    assert pl.graph_status() == 'graph'
    pl.close()
    _, pcfg = hp.configs(pb, **shape)
    pl = hp.make_planner(pb, pcfg)
    pl.plan_begin(pb['state'], seed=9, call=4)
    for it in range(I):
        pl.plan_rollout(it); pl.plan_select(it)
    a, s, n_it = pl.plan_end()                                # (noise_stddev 0: the action is the best candidate's first step)
    assert n_it == ref[2] and s == ref[1]
    np.testing.assert_array_equal(a, ref[0])
    np.testing.assert_array_equal(pl.scores_global().cpu().numpy(), ref[3]); np.testing.assert_array_equal(pl.mu_sigma().cpu().numpy(), ref[4])
    pl.close()
    # a handle fed on the device, its workspace 0xFF before the library saw it
    pl = _device_fed(torch, pb, pcfg)
    _assert_same(ref, _plan_all(pl, pb['state']))
    pl.close()
    # two half-shards, exchanged by hand, reproduce the single rank's first-iteration scores
    halves = []
    for r in range(2):
        _, c2 = hp.configs(pb, world_size=2, rank=r, **shape)
        pl = hp.make_planner(pb, c2)
        pl.plan_begin(pb['state'], seed=9, call=4)
        pl.plan_rollout(0)
        torch.cuda.synchronize()
        halves.append(pl.scores_local().cpu().numpy().copy())
        pl.plan_end()
        pl.close()
    _, c1 = hp.configs(pb, **dict(shape, I=1))
    pl = hp.make_planner(pb, c1)
    pl.plan(pb['state'], seed=9, call=4)
    np.testing.assert_array_equal(np.concatenate(halves), pl.scores_global().cpu().numpy())
    pl.close()


def test_trainer_fed_handle_equals_the_host_fed_one(torch):
    """set_weights_from(trainer): the bf16 image packed on the device from the trainer's workspace is the host packer's, byte for byte,
    and plans the same (the 0xFF fill shows a word the pack kernel did not write)."""
    from ethz_safe_learning_amd import CemPlanner
    from ethz_safe_learning_amd.trainer import CemTrainer
    from tests import handover_cases as hc
    cfg = hc.config(dict(units=32, n_layers=2, ensemble_size=3, particles=3, precision='bf16'))
    tr = CemTrainer(62, 60, 32, 2, 3, batch_size=16)
    tr.set_state(hc.weights(cfg, seed=61))
    H_, D = CemPlanner(cfg), _filled(CemPlanner)(cfg)
    D.set_weights_from(tr)
    H_.set_weights(tr.get_weights())
    h, d = H_.weight_images(), D.weight_images()
    for region in ('wpack', 'bias_h', 'bias_mu', 'bias_var', 'etab'):
        assert h[region].size > 0
        np.testing.assert_array_equal(d[region], h[region], err_msg=region)
    assert not any((v == 0xFFFFFFFF).any() for v in d.values())
    lo = np.full(62, -1.5, F32); hi = np.full(62, 1.5, F32)
    H_.set_normaliser(lo, hi); D.set_normaliser(lo, hi)
    st = np.random.default_rng(4).uniform(0.2, 0.9, 60).astype(F32)
    _assert_same(_plan_all(H_, st), _plan_all(D, st))
    H_.close(); D.close(); tr.close()


# ---- 5. a whole plan against the oracle under the emulation -------------------------------------------------------------------------
@pytest.mark.parametrize('variant', ['cem', 'safe'])
@pytest.mark.parametrize('dims', bc.SHAPES, ids=bc.SHAPE_IDS)
def test_whole_plan_matches_the_oracle_under_the_emulation(torch, dims, variant):
    """N = 128, H = 8, I = 3, k = 12 on explicit noise: iteration count equal, score within 2e-5, action within 1e-5 relative — the
    split test's bars, against do_generate_action with the emulation as its network (seeds: tests/test_bf16_cpu.py)."""
    c = bc.plan_case(dims, variant)
    _, pcfg = hp.configs(c['pb'], variant=variant, noise=0.01, post=0.3, precision='bf16', **bc.PLAN_SHAPE)
    pl = hp.make_planner(c['pb'], pcfg)
    ea, em, eo = c['noise']
    got = pl.plan(c['pb']['state'], eps_act=ea, eps_model=em, eps_out=eo)
    pl.close()
    print('bf16 plan obs %d %s: score %.7f (emulation %.7f), iterations %d (%d)' % (dims[0], variant, got[1], c['ref'][1], got[2], c['ref'][2]))
    bc.check_plan(got, c['ref'], 'obs %d %s' % (dims[0], variant))


# ---- 6. options ride along ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('variant,opts', [
    ('safe', dict(worst_particles=planner.risk_particles(0.2, 5))),
    ('cem', dict(keep_elites=4, action_noise='powerlaw', action_noise_param=1.0)),
], ids=['safe_risk_level', 'cem_keep_elites_noise_beta'])
def test_options_ride_along_and_the_readout_changes_nothing(torch, variant, opts):
    """The options of DESIGN 4.6 - 4.14 sit outside the rollout kernel: a bf16 handle takes them, and its plan with the read-out on
    equals, bit for bit, its plan with the read-out off (the invariance tests/test_gpu_plan_readout.py holds)."""
    import dataclasses
    pb = hp.make_problem(60, 2, 5, 4, seed=12)
    _, pcfg = hp.configs(pb, N=256, H=8, P=5, E=5, k=25, I=3, variant=variant, post=0.3, precision='bf16')
    out = {}
    for readout in (False, True):
        pl = hp.make_planner(pb, dataclasses.replace(pcfg, plan_readout=readout, **opts))
        assert pl.rollout_path() == 'generic'
        out[readout] = _plan_all(pl, pb['state'], seed=5, call=2)
        if readout:
            ro = pl.plan_readout()
            assert ro.sequence.shape == (8, 2) and np.all(np.isfinite(ro.sequence)) and ro.candidate >= 0 and ro.score == np.float32(out[True][1])
        pl.close()
    assert np.isfinite(out[True][1]) and np.all(np.isfinite(out[True][0]))
    _assert_same(out[False], out[True])


def test_batch_handles_refuse_bf16(torch):
    from ethz_safe_learning_amd import BatchCemPlanner
    pb = hp.make_problem(60, 2, 5, 4, seed=12)
    for prec in ('bf16x3', 'bf16'):
        _, pcfg = hp.configs(pb, N=64, H=4, P=5, E=5, k=6, I=1, precision=prec)
        with pytest.raises(_capi.CemError) as e:
            BatchCemPlanner(pcfg, 2)
        assert e.value.status == 2, str(e.value)              # CEM_ERR_UNSUPPORTED


def test_the_automatic_tile_size_plans_like_the_same_size_asked_for(torch):
    """At the headline population the bf16 tile rule and the fp32 rule pick different sizes (three-chunk against one-chunk tiles on 256
    CUs).  Everything a handle derives from its tile size — tile count, pinned tiles, where the sampler runs, launches per iteration —
    must come from the size it runs: the automatic handle reports what a handle asked for that size reports."""
    pb = hp.make_problem(60, 2, 5, 4, seed=12)
    shape = dict(N=2000, H=4, P=5, E=5, k=200, I=1, precision='bf16')
    _, pcfg = hp.configs(pb, **shape)
    auto = hp.make_planner(pb, pcfg)
    rc, tiles = auto.tiles()
    _, pcfg = hp.configs(pb, chunks_per_tile=rc, **shape)
    asked = hp.make_planner(pb, pcfg)
    ip = auto.iteration_plan(0)
    assert ip['chunks_per_tile'] == rc and ip['n_tiles'] == len(tiles) == ip['n_pinned'] and ip['n_segments'] == 1, ip
    assert ip == asked.iteration_plan(0)
    assert auto.launches_per_iteration() == asked.launches_per_iteration()
    _assert_same(_plan_all(auto, pb['state']), _plan_all(asked, pb['state']))
    auto.close(); asked.close()
