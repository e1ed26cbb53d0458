#!/usr/bin/env python3
"""What precision='bf16' costs in accuracy, measured on the device on the plan's own Philox noise at B2 and the shipped safe_cem_mpc
shape (synthetic model), beside the fp32 kernels:
  trajectory   RMS error of the first iteration's unfolded trajectories against the fp64 oracle (oracle/cem_oracle.py) per step;
  scores       the distribution of |score - fp64 oracle score| over the first iteration's candidates;
  plans        over --seeds seeds: how many of the first iteration's n_elite elites differ between a bf16 plan and the fp32 plan of
               the same seed, how often the returned action differs and by how much, and the difference of the returned scores.
No bar is put on any of it: the numbers are written down.  (The committed profiles/bf16_error.json also carries
`kernel_against_its_rounding_model`: the ratios `pytest tests/test_gpu_bf16.py -s` prints, added to the file by hand.)  usage: bf16_error_report.py [--seeds 20] > profiles/bf16_error.json"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402
from ethz_safe_learning_amd import CemPlanner, PlannerConfig, synthetic  # noqa: E402
from oracle import cem_oracle as o  # noqa: E402  (the checker: fp64 reference only)

SHAPES = {'B2': (60, 2, dict(variant='cem', ensemble_size=5, particles=5, n_samples=2000, horizon=30, n_elite=200, iterations=5)),
          'safe_cem_mpc': (60, 2, dict(variant='safe', ensemble_size=15, particles=45, n_samples=500, horizon=8, n_elite=20, iterations=9))}
LEGS = ('fp32', 'bf16')


def planner(pb, obs, act, sh, precision):
    cfg = PlannerConfig(obs_dim=obs, act_dim=act, scorer=pb['scorer'], act_low=pb['low'], act_high=pb['high'], noise_stddev=0.0,
                        posterior_mean_threashold=0.3, stddev_threshold=-1.0, use_graph=False, precision=precision, **sh)
    pl = CemPlanner(cfg)
    pl.set_weights(pb['weights'])
    pl.set_normaliser(pb['inputs_min'], pb['inputs_max'])
    return pl


def quantiles(x):
    x = np.asarray(x, np.float64)
    return dict(median=float(np.median(x)), p90=float(np.quantile(x, 0.9)), p99=float(np.quantile(x, 0.99)), max=float(x.max()), rms=float(np.sqrt(np.mean(x * x))))


def main():
    seeds = int(sys.argv[sys.argv.index('--seeds') + 1]) if '--seeds' in sys.argv else 20
    out = {}
    for shape, (obs, act, sh) in SHAPES.items():
        pb = synthetic.problem(obs, act, sh['ensemble_size'])
        sp = o.ScorerParams(**{k: getattr(pb['scorer'], k) for k in ('goal_slice', 'observe_goal_lidar', 'lidar_max_dist', 'goal_size', 'reward_distance',
                                                                      'reward_goal', 'reward_clip', 'constrain_indicator', 'cost_kinds')})
        P, N, H, E = sh['particles'], sh['n_samples'], sh['horizon'], sh['ensemble_size']
        ocfg = o.PlanConfig(horizon=H, iterations=sh['iterations'], n_samples=N, n_elite=sh['n_elite'], particles=P, ensemble_size=E,
                            variant=sh['variant'], posterior_mean_threashold=0.3)
        pls = {leg: planner(pb, obs, act, sh, leg) for leg in LEGS}
        state = np.asarray(pb['state'], np.float32)
        # ---- first iteration of (seed 1, call 0): trajectories and scores against the fp64 oracle on the dumped Philox noise
        ea, em, _ = pls['fp32'].fill_noise(seed=1, call=0)
        torch.cuda.synchronize()
        ea0, em0 = ea[0].cpu().numpy(), em[0].cpu().numpy()
        lb, ub, mu0, sg0 = o.sampling_params(pb['low'], pb['high'])
        actions = o.sample_actions(np.broadcast_to(mu0, (H, act)), np.broadcast_to(sg0, (H, act)), lb, ub, ea0)
        ref_sc, ref_traj = o.candidate_scores(state.astype(np.float64), actions.astype(np.float64), o.cast_weights(pb['weights'], np.float64),
                                              pb['inputs_min'], pb['inputs_max'], em0, ocfg, sp, return_traj=True)
        s0 = np.broadcast_to(state, (P * N, obs)).copy()
        a_b = np.tile(actions.astype(np.float32), (P, 1, 1))
        res = {}
        for leg in LEGS:
            pl = pls[leg]
            traj = pl.unfold_sequences(s0, a_b, eps_model=em[0]).cpu().numpy().astype(np.float64)
            per_step = [float(np.sqrt(np.mean((traj[:, t] - ref_traj[:, t]) ** 2))) for t in range(1, H + 1)]
            pl.plan_begin(state, seed=1, call=0)
            pl.plan_rollout(0)
            torch.cuda.synchronize()
            sc = pl.scores_local().cpu().numpy().astype(np.float64)
            pl.plan_end()
            res[leg] = dict(trajectory_rms_error_per_step=per_step, score_abs_error=quantiles(np.abs(sc - ref_sc)),
                            score_abs_error_over_1e_3=float(np.mean(np.abs(sc - ref_sc) > 1e-3)))
        res['state_rms_move_per_step'] = float(np.sqrt(np.mean((ref_traj[:, 1:] - ref_traj[:, :-1]) ** 2)))
        res['score_spread_std'] = float(np.std(ref_sc[np.isfinite(ref_sc)]))
        # ---- plans of the same seed on both precisions
        elite_diff, act_diff, score_diff = [], [], []
        for seed in range(seeds):
            got = {}
            for leg in LEGS:
                pl = pls[leg]
                pl.plan_begin(state, seed=100 + seed, call=0)
                pl.plan_rollout(0); pl.plan_select(0)
                torch.cuda.synchronize()
                elite = set(pl.elite_idx().cpu().numpy().tolist())
                pl.plan_end()
                a, s, _ = pl.plan(state, seed=100 + seed, call=0)
                got[leg] = (elite, a, s)
            elite_diff.append(len(got['fp32'][0] - got['bf16'][0]))
            act_diff.append(float(np.abs(got['fp32'][1] - got['bf16'][1]).max()))
            score_diff.append(float(got['bf16'][2] - got['fp32'][2]))
        res['plans'] = dict(seeds=seeds, n_elite=sh['n_elite'], first_iteration_elites_differing=elite_diff,
                            elite_sets_differ_fraction=float(np.mean(np.asarray(elite_diff) > 0)),
                            mean_elites_differing=float(np.mean(elite_diff)),
                            returned_action_differs_fraction=float(np.mean(np.asarray(act_diff) > 0)),
                            returned_action_max_abs_diff=quantiles(act_diff), returned_score_diff_bf16_minus_fp32=quantiles(np.abs(score_diff)),
                            returned_score_diff_mean_signed=float(np.mean(score_diff)))
        for pl in pls.values():
            pl.close()
        out[shape] = res
        sys.stderr.write('%s done\n' % shape)
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
