"""The task scorer (cem_mpc.h "Task scorers", cem_planner_set_task): a plain float64 evaluation of its contract, the
tasks, random and crafted trajectories its tests share, and the double integrator of the closed-loop test.

planner.task_objective is the bit-exact float32 restatement of the kernel; objective_f64 here is the contract written down the
obvious way, in float64 and NumPy's own summation order — what the mirror is measured against on the CPU."""
import numpy as np

from ethz_safe_learning_amd.planner import PlannerConfig, QuadraticTask, ScorerConfig

NEAR = 1e-4                      # a comparison whose operands are closer than this may resolve either way between float32 and float64
# (O, A, H, rows, P) of the kernel-alone tests: one lane quad and a single step; O % 4 != 0 (the element path) with three blocks of rows
# and a partial last one; the shipped observation width on the 16-byte path; two quads per lane (O > 64) with a wide action
SHAPES = [(5, 1, 1, 3, 1), (57, 2, 7, 150, 3), (60, 2, 30, 150, 3), (100, 12, 9, 66, 3)]


def task_for(O, A, seed=0, clip=True):
    """A task with every table in use: q >= 0, g, c of either sign, a goal on features 0 and 1 (g = 0 there, radius 0.5: R2 = 0.25
    exactly), a box of +-2.5 on most features (the rest unbounded), rho > 0, a goal bonus and (clip) a reward clip of 0.55 O — near the
    median of phi for standard normal states, so that about half of the steps are clipped."""
    rng = np.random.default_rng(1000 + seed)
    q = rng.uniform(0.0, 1.0, O).astype(np.float32)
    g = rng.normal(0.0, 0.3, O).astype(np.float32)
    g[:2] = 0.0
    c = rng.normal(0.0, 0.1, O).astype(np.float32)
    m = np.zeros(O, np.float32)
    m[:2] = 1.0
    lo = np.full(O, -2.5, np.float32)
    hi = np.full(O, 2.5, np.float32)
    lo[3::5] = -np.inf
    hi[4::5] = np.inf
    rho = rng.uniform(0.05, 0.5, A).astype(np.float32)
    return QuadraticTask(q=q, g=g, c=c, goal_mask=m, lo=lo, hi=hi, rho=rho, goal_radius=0.5, reward_goal=3.0,
                         reward_clip=float(np.float32(0.55 * O)) if clip else 0.0)


def random_case(O, A, H, rows, P, seed=0):
    """(traj [rows, H + 1, O], actions [rows / P, H, A]): standard normal states (near holds on about one state in eight), uniform actions."""
    rng = np.random.default_rng(2000 + seed)
    tr = rng.standard_normal((rows, H + 1, O)).astype(np.float32)
    act = rng.uniform(-1.0, 1.0, (rows // P, H, A)).astype(np.float32)
    return tr, act


def clear_thresholds(tr, task, width=1e-3):
    """Moves every value of a random tensor that lies within `width` of a bound, and every state whose goal distance lies within
    `width` of R2, well away from it (in place): what is left resolves the same way in float32 and float64."""
    f = np.float32
    O = tr.shape[2]
    for b in ('lo', 'hi'):
        bound = np.broadcast_to(np.asarray(getattr(task, b), f), (O,))
        with np.errstate(invalid='ignore'):
            close = np.abs(tr - bound) < width
        tr[close] = f(0.0)
    g = np.broadcast_to(np.asarray(task.g, np.float64), (O,))
    m = np.broadcast_to(np.asarray(task.goal_mask, np.float64), (O,))
    nsum = (m * (tr.astype(np.float64) - g) ** 2).sum(axis=2)
    r2 = float(f(task.goal_radius)) ** 2
    tr[np.abs(nsum - r2) < width, 0] = f(2.0)
    return tr


def craft(tr, task, boundaries=True):
    """Crafted rows over a random trajectory tensor, in place; returns {name: row}.  boundaries=False leaves out the rows that sit ON a
    threshold (they are for the bit-exact comparison with the mirror, not for the float64 one)."""
    rows, H1, O = tr.shape
    H = H1 - 1
    f = np.float32
    tb = {k: np.broadcast_to(np.asarray(getattr(task, k), f), (O,)) for k in ('lo', 'hi')}
    out = {}
    bounded = int(np.nonzero(np.isfinite(tb['lo']) & np.isfinite(tb['hi']))[0][-1])     # a feature with both bounds (not 0 / 1: the goal's)
    t1 = min(1, H)

    def calm(r):                     # inside the box everywhere, far from the goal: no cost, never near
        tr[r] = np.clip(tr[r], -2.0, 2.0)
        tr[r, :, 0] = f(2.0)
    if boundaries and rows > 2:
        calm(0); tr[0, 0, bounded] = tb['lo'][bounded]; tr[0, t1, bounded] = tb['hi'][bounded]; out['on_bounds'] = 0
        calm(1); tr[1, 0, bounded] = np.nextafter(tb['lo'][bounded], f(-np.inf)); out['ulp_below_lo'] = 1
        calm(2); tr[2, 0, bounded] = np.nextafter(tb['hi'][bounded], f(np.inf)); out['ulp_above_hi'] = 2
    if boundaries and rows > 4:
        calm(3); tr[3, 0, 0] = f(0.5); tr[3, 0, 1] = f(0.0); out['near_exactly'] = 3          # 0.25 + 0 == R2
        calm(4); tr[4, 0, 0] = np.nextafter(f(0.5), f(1.0)); tr[4, 0, 1] = f(0.0); out['near_ulp_outside'] = 4
    if rows > 7 and H >= 3:
        calm(5); tr[5, 0, 0] = f(0.1); tr[5, 0, 1] = f(0.1); out['goal_at_0'] = 5
        calm(6); tr[6, H - 1, 0] = f(0.1); tr[6, H - 1, 1] = f(0.1); out['goal_at_last_step'] = 6
        calm(7); out['goal_never'] = 7
    if boundaries and rows > 8 and H >= 3:
        calm(8); tr[8, 2, bounded] = f(np.nan); out['nan_feature'] = 8
    return out


def objective_f64(traj, actions, task, variant):
    """The contract in float64: (returns [rows], cost bytes [H, rows] or None, done step [rows] (H: never), margin) — margin is the
    smallest distance of any comparison operand to its threshold (near's sum to R2 where a goal is set, every bounded feature to its
    bound)."""
    tr = np.asarray(traj, np.float64)
    act = np.asarray(actions, np.float64)
    rows, H1, O = tr.shape
    N, H, A = act.shape
    tb = {k: v.astype(np.float64) for k, v in task.tables(O, A).items()}
    r2 = float(np.float32(task.goal_radius)) ** 2
    d = tr - tb['g']
    phi = (tb['q'] * d * d - tb['c'] * tr).sum(axis=2)
    nsum = (tb['goal_mask'] * d * d).sum(axis=2)
    has_goal = r2 > 0 and variant != 'cost'
    near = (nsum <= r2) & has_goal
    viol = ((tr < tb['lo']) | (tr > tb['hi'])).any(axis=2)
    u = (tb['rho'] * act * act).sum(axis=2)[np.arange(rows) % N]
    clip = float(task.reward_clip) if task.reward_clip > 0 else np.inf
    margin = np.inf
    if has_goal:
        margin = min(margin, float(np.abs(nsum[:, :H] - r2).min()))
    with np.errstate(invalid='ignore'):
        for b in ('lo', 'hi'):
            fin = np.isfinite(tb[b])
            if fin.any():
                margin = min(margin, float(np.nanmin(np.abs(tr[:, :H, fin] - tb[b][fin]))))
    safe = variant != 'cem'
    cum = np.zeros(rows)
    done = np.zeros(rows, bool)
    done_step = np.full(rows, H)
    costs = np.zeros((H, rows), np.uint8) if safe else None
    for t in range(H):
        ga = near[:, t]
        r = -phi[:, t + 1] - u[:, t] + np.where(ga, float(task.reward_goal), 0.0)
        r = np.clip(r, -clip, clip)
        done_step = np.where(ga & (done_step == H), t, done_step)
        if safe:
            done = done | ga
            costs[t] = viol[:, t] & ~done
            cum = cum + np.where(done, 0.0, r)
        else:
            cum = cum + np.where(done, 0.0, r)
            done = done | ga
    return cum, costs, done_step, margin


def kernel_handle_config(O, A, P, variant):
    """A small handle whose only purpose is cem_task_score at (O, A, P): the op takes its own row count and horizon."""
    return PlannerConfig(obs_dim=O, act_dim=A, ensemble_size=1, particles=P, n_samples=8, horizon=2, n_elite=2, iterations=1,
                         scorer=ScorerConfig(goal_slice=(0, 1)), act_low=[-1.0] * A, act_high=[1.0] * A, units=32, n_layers=2, variant=variant)


# ---------------------------------------------------------------------------------------------------------------------------------
# The double integrator: obs (pos, vel), one action; pos' = pos + DT vel, vel' = vel + DT a.  The ensemble weights are set by hand to
# these dynamics: the network sees x = (s, a) unscaled (scale_features off), its first layer holds relu(+x_i) and relu(-x_i) of every
# input, the later layers pass the six units through (they are >= 0), the mean head recombines them into the state CHANGE, the variance
# head's bias is driven to softplus's floor.
# ---------------------------------------------------------------------------------------------------------------------------------
DT = 0.1
UNITS = 16


def integrator_weights(E, n_layers=2):
    W0 = np.zeros((3, UNITS), np.float32)
    for i in range(3):
        W0[i, 2 * i], W0[i, 2 * i + 1] = 1.0, -1.0
    eye = np.zeros((UNITS, UNITS), np.float32)
    eye[:6, :6] = np.eye(6, dtype=np.float32)
    Wmu = np.zeros((UNITS, 2), np.float32)
    Wmu[2, 0], Wmu[3, 0] = DT, -DT                   # d pos = DT vel
    Wmu[4, 1], Wmu[5, 1] = DT, -DT                   # d vel = DT a
    one = dict(W=[W0] + [eye.copy() for _ in range(n_layers - 1)], b=[np.zeros(UNITS, np.float32) for _ in range(n_layers)],
               W_mu=Wmu, b_mu=np.zeros(2, np.float32), W_var=np.zeros((UNITS, 2), np.float32), b_var=np.full(2, -40.0, np.float32))
    return [dict((k, [a.copy() for a in v] if isinstance(v, list) else v.copy()) for k, v in one.items()) for _ in range(E)]


def integrator_step(s, a):
    """The exact dynamics, float32 like the model: s [.., 2], a [..] -> s'."""
    s = np.asarray(s, np.float32)
    a = np.asarray(a, np.float32)
    return np.stack([s[..., 0] + np.float32(DT) * s[..., 1], s[..., 1] + np.float32(DT) * a], axis=-1).astype(np.float32)


VEL_BOX = 1.0
INTEGRATOR_TASK = QuadraticTask(q=[1.0, 0.1], g=0.0, lo=[-np.inf, -VEL_BOX], hi=[np.inf, VEL_BOX], rho=0.01)


def stage_cost(s):
    """q (s - g)^2 of INTEGRATOR_TASK at a state, float64."""
    s = np.asarray(s, np.float64)
    return float(1.0 * s[0] ** 2 + 0.1 * s[1] ** 2)


# the closed loop of the double-integrator test: from pos 1 at rest, STEPS decisions of a CemMpc(N, H, I, k, P) plan
INTEGRATOR = dict(N=64, H=10, I=3, k=8, P=2, E=2, steps=40)


# reference_closed_loop over seeds 0 .. 4, measured on the CPU (tests/test_task_cpu.py holds them to it): the worst final stage cost and
# the largest |vel| — inside the box, so the reference's worst violation of it is 0
REFERENCE_WORST_STAGE_COST = 2.61e-4
REFERENCE_WORST_SPEED = 0.911


def reference_closed_loop(seed):
    """A NumPy CEM on the same model: candidates sampled like the policy's (oracle.sample_actions from a seeded generator), rolled out
    with the exact dynamics (the model's noise is off: every particle of a candidate is the same row), scored by planner.task_objective
    and the particle mean, ranked and refitted by the oracle's select_and_refit.  -> (final stage cost, largest |vel| on the executed
    trajectory)."""
    from oracle import cem_oracle as o
    from ethz_safe_learning_amd.planner import task_objective
    c = INTEGRATOR
    N, H, I, P = c['N'], c['H'], c['I'], c['P']
    cfg = o.PlanConfig(horizon=H, iterations=I, n_samples=N, n_elite=c['k'], particles=P, ensemble_size=c['E'], sampling_propagation=False,
                       scale_features=False)
    f = np.float32
    rng = np.random.default_rng(seed)
    lb, ub, mu0, sigma0 = o.sampling_params([-1.0], [1.0])
    s = np.array([1.0, 0.0], f)
    vmax = 0.0
    for _ in range(c['steps']):
        mu = np.broadcast_to(mu0, (H, 1)).astype(f).copy()
        sigma = np.broadcast_to(sigma0, (H, 1)).astype(f).copy()
        best, best_score = np.zeros(1, f), f(-np.inf)
        for it in range(I):
            actions = o.sample_actions(mu, sigma, lb, ub, rng.standard_normal((N, H, 1)).astype(f))
            traj = np.zeros((N, H + 1, 2), f)
            traj[:, 0] = s
            for t in range(H):
                traj[:, t + 1] = integrator_step(traj[:, t], actions[:, t, 0])
            ret, _ = task_objective(np.tile(traj, (P, 1, 1)), actions, INTEGRATOR_TASK, 'cem')
            scores = ret.reshape(P, N).sum(axis=0, dtype=f) / f(P)
            mu, sigma, best, best_score, _, _ = o.select_and_refit(scores, actions, mu, sigma, best, best_score, cfg)
        s = integrator_step(s, best[0])
        vmax = max(vmax, abs(float(s[1])))
    return stage_cost(s), vmax
