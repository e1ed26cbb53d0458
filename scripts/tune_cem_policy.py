#!/usr/bin/env python3
"""Counterpart of the reference's scripts/tune_cem_policy.py (:56-137): train, then grid-search the CEM planner over
horizon x (proposals, iterations) x elite ratio by swapping ``agent.policy`` for fresh ``CemMpc`` objects and evaluating
each.  Every distinct (H, I, N, k) is a new planner handle (the reference re-traces its tf.function); handles are cached
by shape.  Results go to <log_dir>/grid_search.json (and scores.svg / costs.svg when matplotlib is installed).

  python scripts/tune_cem_policy.py --config_dir ethz_safe_learning_amd/config --config_basename smoke.yaml \
         --eval_steps 300 --eval_episode_length 300

--parallel_episodes K (K > 1) evaluates each configuration on K PointGoal environments of distinct seeds stepped in lockstep
(BaseAgent.sample_trajectories_lockstep): one batched plan (CemMpc.generate_actions) per decision for all of them.  The default, 1,
is the serial evaluation above.

--elite_temperature T [T ...] adds a grid axis: every configuration is also evaluated with the score-weighted refit at each temperature
(CemMpc(elite_temperature=T); the word `none` stands for the uniform refit).  Without the flag the grid and its records are the reference's.

--noise_beta B [B ...] adds a grid axis in the same way: every configuration is also evaluated with power-law action noise of each
spectral exponent (CemMpc(noise_beta=B); the word `none` stands for the reference's white noise).

--keep_elites F [F ...] adds a grid axis in the same way: every configuration is also evaluated with the best fraction F of its elites
carried from iteration to iteration (CemMpc(keep_elites=F); the word `none` stands for the reference's resampling of every candidate).

--population_decay F [F ...] adds a grid axis in the same way: every configuration is also evaluated with iteration i sampling about
n_samples / F**i candidates (CemMpc(population_decay=F); the word `none` stands for the reference's full population in every iteration).
Such a policy plans one state at a time: not together with --parallel_episodes.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'scripts'))

HORIZONS = [8, 10, 12, 15]
PROPOSALS_WITH_ITERATIONS = [(100, 15), (150, 10), (300, 5)]
ELITE_RATIOS = [0.05, 0.1, 0.2]


WARM_KWARGS = ('warm_start', 'warm_shift', 'warm_tail', 'warm_sigma', 'warm_sigma_floor', 'elite_temperature', 'noise_beta', 'keep_elites', 'shift_elites',
               'population_decay', 'min_population', 'mean_candidate')


def make_new_policy(model, environment, horizon, iterations, n_samples, elite_ratio, policy_kwargs):
    from ethz_safe_learning_amd.simba.policies import CemMpc
    return CemMpc(model=model, environment=environment, horizon=horizon, iterations=iterations, n_samples=n_samples,
                  n_elite=round(elite_ratio * n_samples), particles=policy_kwargs['particles'],
                  stddev_threshold=policy_kwargs['stddev_threshold'], noise_stddev=policy_kwargs['noise_stddev'],
                  smoothing=policy_kwargs['smoothing'], seed=policy_kwargs.get('seed', 0),
                  **{k: policy_kwargs[k] for k in WARM_KWARGS if k in policy_kwargs})      # (--warm_start, or the user's own config)


def make_parallel_environments(params, k, seed):
    """K environments of the experiment's task with distinct seeds, for the lockstep evaluation."""
    from ethz_safe_learning_amd.simba.environment_utils.environment_factory import make_environment
    return [make_environment(params, seed=seed + 1 + i) for i in range(k)]


def evaluate_lockstep(trainer, environments, eval_steps, eval_episode_length):
    """trainer.evaluate_agent's metrics over episodes of several environments stepped side by side."""
    from ethz_safe_learning_amd.simba.infrastructure.trainer import _returns_and_costs
    agent = trainer.agent
    trajectories, _ = agent.sample_trajectories_lockstep(environments, agent.policy, eval_steps, eval_episode_length)
    returns, costs = _returns_and_costs(trajectories)
    return dict(training_rl_objective=returns.mean(), sum_rewards_stddev=returns.std(), sum_costs_mean=costs.mean(),
                sum_costs_stddev=costs.std())


def grid_search(trainer, env, params, eval_steps, eval_episode_length, horizons=HORIZONS,
                proposals_with_iterations=PROPOSALS_WITH_ITERATIONS, elite_ratios=ELITE_RATIOS, parallel_envs=None,
                elite_temperatures=None, noise_betas=None, keep_elites=None, population_decays=None, replan_everys=None):
    """elite_temperatures: None (the reference's grid) or a list of temperatures, None among them for the uniform refit — a fourth axis.
    noise_betas: None or a list of power-law exponents, None among them for white noise — a further axis.
    keep_elites: None or a list of kept fractions of n_elite, None among them for no carry-over — a further axis.
    population_decays: None or a list of decay factors >= 1, None among them for the full population — a further axis.
    replan_everys: None or a list of integers r >= 1, None among them for a plan at every decision — a further axis; a warm-started
    policy's warm_shift follows r (the carried distribution moves as many steps as were executed)."""
    from ethz_safe_learning_amd.simba.infrastructure.logging_utils import logger
    agent = trainer.agent
    results = []
    for horizon in horizons:
        for n_samples, iterations in proposals_with_iterations:
            for ratio, temperature, beta, keep, decay, every in [(r, t, b, f, g, e) for r in elite_ratios for t in (elite_temperatures or [None])
                                                                 for b in (noise_betas or [None]) for f in (keep_elites or [None])
                                                                 for g in (population_decays or [None]) for e in (replan_everys or [None])]:
                kwargs = params['policies']['cem_mpc']
                if elite_temperatures:
                    kwargs = dict(kwargs, elite_temperature=temperature)
                if noise_betas:
                    kwargs = dict(kwargs, noise_beta=beta)
                if keep_elites:
                    kwargs = dict(kwargs, keep_elites=keep)
                if population_decays:
                    kwargs = dict(kwargs, population_decay=decay)
                if replan_everys and every is not None:
                    kwargs = dict(kwargs, replan_every=every)
                    if kwargs.get('warm_start') or kwargs.get('shift_elites'):
                        kwargs['warm_shift'] = every
                agent.policy = make_new_policy(agent.model, env, horizon, iterations, n_samples, ratio, kwargs)
                t0 = time.perf_counter()
                if parallel_envs:
                    m = evaluate_lockstep(trainer, parallel_envs, eval_steps, eval_episode_length)
                else:
                    m = trainer.evaluate_agent(eval_steps, eval_episode_length)
                rec = dict(horizon=horizon, n_samples=n_samples, iterations=iterations, elite_ratio=ratio,
                           n_elite=agent.policy.elite, score_mean=float(m['training_rl_objective']),
                           score_std=float(m['sum_rewards_stddev']), cost_mean=float(m['sum_costs_mean']),
                           cost_std=float(m['sum_costs_stddev']), seconds=time.perf_counter() - t0)
                if elite_temperatures:
                    rec['elite_temperature'] = temperature
                if noise_betas:
                    rec['noise_beta'] = beta
                if keep_elites:
                    rec['keep_elites'] = keep
                if population_decays:
                    rec['population_decay'] = decay
                if replan_everys:
                    rec['replan_every'] = every
                logger.info('H=%d (N,I)=(%d,%d) elite %.2f: score %.3f +- %.3f, cost %.3f +- %.3f', horizon, n_samples, iterations,
                            ratio, rec['score_mean'], rec['score_std'], rec['cost_mean'], rec['cost_std'])
                results.append(rec)
    return results


def main(argv=None):
    import train as train_script
    ap = argparse.ArgumentParser()
    ap.add_argument('--name', type=str, default='')
    ap.add_argument('--log_dir', type=str, default='experiments')
    ap.add_argument('--log_level', type=str, default='INFO')
    ap.add_argument('--config_dir', type=str, required=True)
    ap.add_argument('--config_basename', type=str, required=True)
    ap.add_argument('--cuda_device', type=str, default='0')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--eval_steps', type=int, default=7000)                 # tune_cem_policy.py:116
    ap.add_argument('--eval_episode_length', type=int, default=1000)
    ap.add_argument('--quick', action='store_true', help='2 x 2 x 2 corner of the grid (tests)')
    ap.add_argument('--parallel_episodes', type=int, default=1,
                    help='K > 1: evaluate on K environments of distinct seeds in lockstep, one batched plan per decision')
    ap.add_argument('--warm_start', action='store_true',
                    help="every grid point's policy warm-starts its plans (CemMpc(warm_start=True, warm_sigma='keep')): run the search both ways")
    ap.add_argument('--elite_temperature', type=str, nargs='+', default=None, metavar='T',
                    help="a grid axis of softmax refit temperatures (CemMpc(elite_temperature=T)); 'none' = the uniform refit")
    ap.add_argument('--noise_beta', type=str, nargs='+', default=None, metavar='B',
                    help="a grid axis of power-law action-noise exponents (CemMpc(noise_beta=B)); 'none' = the reference's white noise")
    ap.add_argument('--keep_elites', type=str, nargs='+', default=None, metavar='F',
                    help="a grid axis of kept elite fractions (CemMpc(keep_elites=F)); 'none' = every candidate resampled, as the reference does")
    ap.add_argument('--population_decay', type=str, nargs='+', default=None, metavar='F',
                    help="a grid axis of population decay factors (CemMpc(population_decay=F)); 'none' = n_samples candidates in every iteration")
    ap.add_argument('--replan_every', type=str, nargs='+', default=None, metavar='R',
                    help="a grid axis of decisions per plan (CemMpc(replan_every=R), 1 <= R <= the smallest horizon of the grid); 'none' = a plan at "
                         "every decision, as the reference does")
    args = ap.parse_args(argv)
    if args.replan_every and args.parallel_episodes > 1:
        ap.error('--replan_every keeps one sequence per policy (CemMpc.generate_actions refuses it): not with --parallel_episodes')
    if args.parallel_episodes < 1:
        ap.error('--parallel_episodes must be at least 1')
    if args.population_decay and args.parallel_episodes > 1:
        ap.error('--population_decay plans one state at a time (CemMpc.generate_actions refuses it): not with --parallel_episodes')
    from ethz_safe_learning_amd.config.config import load_config_or_die
    params = load_config_or_die(args.config_dir, args.config_basename)
    trainer = train_script.main(['--config_dir', args.config_dir, '--config_basename', args.config_basename, '--log_dir', args.log_dir,
                                 '--name', args.name, '--seed', str(args.seed), '--log_level', args.log_level,
                                 '--cuda_device', args.cuda_device])
    if args.warm_start:
        params['policies']['cem_mpc'] = dict(params['policies']['cem_mpc'], warm_start=True, warm_sigma='keep')
    grid = dict(horizons=HORIZONS[:2], proposals_with_iterations=PROPOSALS_WITH_ITERATIONS[1:], elite_ratios=ELITE_RATIOS[:2]) if args.quick else {}
    if args.elite_temperature:
        grid['elite_temperatures'] = [None if t.lower() == 'none' else float(t) for t in args.elite_temperature]
    if args.noise_beta:
        grid['noise_betas'] = [None if b.lower() == 'none' else float(b) for b in args.noise_beta]
    if args.keep_elites:
        grid['keep_elites'] = [None if f.lower() == 'none' else float(f) for f in args.keep_elites]
    if args.population_decay:
        grid['population_decays'] = [None if g.lower() == 'none' else float(g) for g in args.population_decay]
    if args.replan_every:
        grid['replan_everys'] = [None if r.lower() == 'none' else int(r) for r in args.replan_every]
        lowest = min(grid.get('horizons', HORIZONS))
        if any(r is not None and not 1 <= r <= lowest for r in grid['replan_everys']):
            ap.error('--replan_every must lie in [1, %d], the smallest horizon of the grid' % lowest)
    if args.parallel_episodes > 1:
        grid['parallel_envs'] = make_parallel_environments(params, args.parallel_episodes, args.seed)
    results = grid_search(trainer, trainer.environment, params, args.eval_steps, args.eval_episode_length, **grid)
    out_dir = trainer.training_logger.log_dir or args.log_dir
    with open(os.path.join(out_dir, 'grid_search.json'), 'w') as fh:
        json.dump(results, fh, indent=1)
    try:
        import matplotlib
        matplotlib.use('Agg')
        import matplotlib.pyplot as plt
        for key, cmap in (('score_mean', 'Blues'), ('cost_mean', 'Reds')):
            hs = sorted({r['horizon'] for r in results})
            fig, axes = plt.subplots(1, len(hs), sharey='all', figsize=(3 * len(hs), 3))
            for ax, h in zip(np.atleast_1d(axes), hs):
                rows = [r for r in results if r['horizon'] == h]
                ne = len({r['elite_ratio'] for r in rows})
                ax.pcolor(np.array([r[key] for r in rows]).reshape(-1, ne), cmap=cmap)
                ax.set_title('H=%d' % h)
            fig.savefig(os.path.join(out_dir, key + '.svg'))
    except ImportError:
        pass
    return results


if __name__ == '__main__':
    main()
