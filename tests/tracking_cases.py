"""The tracking task (cem_mpc.h "Tracking tasks", cem_planner_set_task_tracking): a plain float64 evaluation of its
contract, the tasks, clocks, random and crafted trajectories its tests share, and the closed loop that follows a sine.

planner.tracking_objective is the bit-exact float32 restatement of the kernel; tracking_f64 here is the contract written down the
obvious way, in float64 and NumPy's own summation order — what the mirror is measured against on the CPU."""
import numpy as np

from ethz_safe_learning_amd.planner import TrackingTask
from tests import task_cases as tc

SHAPES = tc.SHAPES
# the largest |mirror - float64| / max(1, |float64|) over the returns of test_tracking_cpu.test_mirror_against_float64's cases, measured on
# the CPU (returns down to -1.6e3: sums of up to 30 steps of up to 100 feature terms in float32); that test's bar is twice this
MIRROR_ERROR_MEASURED = 2.76e-7


def clock_cases(H):
    """(T, k0): one row; a row per state; the last three states hold the last row; a short table from its start; every state holds the
    last row."""
    return [(1, 0), (H + 1, 0), (H + 1, 3), (3, 0), (4, 9)]


def row_of(T, k0, H):
    """The reference row of every state s_0 .. s_H."""
    return np.minimum(k0 + np.arange(H + 1), T - 1)


def tracking_task_for(O, A, T, seed=0, clip=True, terminal=True, rate=True):
    """task_cases.task_for's tables around a reference of T rows: the goal features 0 and 1 of every row are exact binary fractions
    (eighths and quarters, within +-0.25: the crafted "near exactly" rows subtract them exactly), the others normal(0, 0.3); the LAST row
    is 0.5 away from where the others lie on every feature but the goal's, where it holds (0.375, -0.375): it differs from all the
    others.  terminal: qT = 4 q on even features, 0.25 q on odd ones; rate: kappa in [0.1, 0.6]."""
    base = tc.task_for(O, A, seed, clip)
    rng = np.random.default_rng(3000 + seed)
    ref = rng.normal(0.0, 0.3, (T, O)).astype(np.float32)
    j = np.arange(T)
    ref[:, 0] = ((j % 5) - 2) / 8.0
    if O > 1:
        ref[:, 1] = ((j % 3) - 1) / 4.0
    ref[-1, 2:] += np.float32(0.5)
    ref[-1, :2] = np.array([0.375, -0.375], np.float32)[:min(O, 2)]
    q = np.asarray(base.q, np.float32)
    qT = (q * np.where(np.arange(O) % 2 == 0, 4.0, 0.25)).astype(np.float32) if terminal else None
    kappa = rng.uniform(0.1, 0.6, A).astype(np.float32) if rate else None
    return TrackingTask(reference=ref, q=q, c=base.c, goal_mask=base.goal_mask, lo=base.lo, hi=base.hi, rho=base.rho,
                        goal_radius=base.goal_radius, reward_goal=base.reward_goal, reward_clip=base.reward_clip, terminal_weights=qT,
                        action_rate=kappa)


def prev_action_for(A, seed=0):
    """A non-zero a_{-1} inside the action box."""
    return np.random.default_rng(4000 + seed).uniform(-1.0, 1.0, A).astype(np.float32)


def clear_thresholds(tr, task, k0, width=1e-3):
    """task_cases.clear_thresholds with every state's goal distance measured against the row it is compared with (in place)."""
    f = np.float32
    rows, H1, O = tr.shape
    for b in ('lo', 'hi'):
        bound = np.broadcast_to(np.asarray(getattr(task, b), f), (O,))
        with np.errstate(invalid='ignore'):
            close = np.abs(tr - bound) < width
        tr[close] = f(0.0)
    ref = np.asarray(task.reference, np.float64)
    g = ref[row_of(ref.shape[0], k0, H1 - 1)]                                   # [H + 1, O]
    m = np.broadcast_to(np.asarray(task.goal_mask, np.float64), (O,))
    nsum = (m * (tr.astype(np.float64) - g) ** 2).sum(axis=2)
    r2 = float(f(task.goal_radius)) ** 2
    tr[np.abs(nsum - r2) < width, 0] = f(2.0)
    return tr


def craft(tr, act, task, k0, prev_action, boundaries=True):
    """Crafted rows over random trajectories and actions, in place; returns {name: row}.  boundaries=False leaves out the rows that sit
    ON a threshold (they are for the bit-exact comparison with the mirror, not for the float64 one).  Row r is candidate r's first
    particle (r < N)."""
    rows, H1, O = tr.shape
    H = H1 - 1
    N = act.shape[0]
    f = np.float32
    ref = np.asarray(task.reference, f)
    g = ref[row_of(ref.shape[0], k0, H)]                                         # the row of every state
    lo, hi = (np.broadcast_to(np.asarray(getattr(task, k), f), (O,)) for k in ('lo', 'hi'))
    out = {}
    bounded = int(np.nonzero(np.isfinite(lo) & np.isfinite(hi))[0][-1])          # a feature with both bounds (not 0 / 1: the goal's)
    t1 = min(1, H)

    def calm(r):                     # inside the box everywhere, far from every row's goal: no cost, never near
        tr[r] = np.clip(tr[r], -2.0, 2.0)
        tr[r, :, 0] = f(2.0)
    if boundaries and rows > 2:
        calm(0); tr[0, 0, bounded] = lo[bounded]; tr[0, t1, bounded] = hi[bounded]; out['on_bounds'] = 0
        calm(1); tr[1, 0, bounded] = np.nextafter(lo[bounded], f(-np.inf)); out['ulp_below_lo'] = 1
        calm(2); tr[2, 0, bounded] = np.nextafter(hi[bounded], f(np.inf)); out['ulp_above_hi'] = 2
    if boundaries and rows > 4:
        # against the row of s_1 where the plan has one (a MOVING row): d = 0.5 exactly on feature 0, 0 on feature 1: 0.25 + 0 == R2
        # (away from zero, so that the state's ulp is the difference's: |s| >= 0.5)
        st = t1 if H > 1 else 0
        away = f(0.5) if g[st, 0] >= 0 else f(-0.5)
        calm(3); tr[3, st, 0] = g[st, 0] + away; tr[3, st, 1] = g[st, 1]; out['near_exactly'] = 3
        calm(4); tr[4, st, 0] = np.nextafter(f(g[st, 0] + away), f(8.0) * away); tr[4, st, 1] = g[st, 1]; out['near_ulp_outside'] = 4
        assert f(tr[3, st, 0] - g[st, 0]) == away and abs(f(tr[4, st, 0] - g[st, 0])) > f(0.5)
        out['near_state'] = st
    if rows > 7 and H >= 3:
        calm(5); tr[5, 0, :2] = g[0, :2] + f(0.1); out['goal_at_0'] = 5
        calm(6); tr[6, H - 1, :2] = g[H - 1, :2] + f(0.1); out['goal_at_last_step'] = 6
        calm(7); out['goal_never'] = 7
    if boundaries and rows > 8 and H >= 3:
        calm(8); tr[8, 2, bounded] = f(np.nan); out['nan_feature'] = 8
    if rows > 12 and N > 12 and H >= 3:
        # on the reference everywhere but for ONE deviation, at s_H (weighted by qT) or at s_{H-1} (by q); the same actions
        for r, st in ((9, H), (10, H - 1)):
            tr[r] = g; tr[r, :, 0] = f(2.0); tr[r, st, bounded] = g[st, bounded] + f(0.5)
        act[10] = act[9]
        out['deviation_at_H'], out['deviation_before_H'] = 9, 10
        # a_0 == a_{-1} exactly (the first step's rate term is +0), later steps differ
        calm(11); act[11, 0] = prev_action; out['first_action_is_previous'] = 11
        assert not np.array_equal(act[11, 1], act[11, 0])
    return out


def tracking_f64(traj, actions, task, variant, k0=0, prev_action=None):
    """The contract in float64: (returns [rows], cost bytes [H, rows] or None, done step [rows] (H: never), margin) — margin is the
    smallest distance of any comparison operand to its threshold (near's sum to R2 where a goal is set, every bounded feature to its
    bound)."""
    tr = np.asarray(traj, np.float64)
    act = np.asarray(actions, np.float64)
    rows, H1, O = tr.shape
    N, H, A = act.shape
    tb = {k: v.astype(np.float64) for k, v in task.tables(O, A).items()}
    g = tb['reference'][row_of(tb['reference'].shape[0], k0, H)]                 # [H + 1, O]
    w = np.tile(tb['q'], (H1, 1))
    w[H] = tb['q_terminal']
    r2 = float(np.float32(task.goal_radius)) ** 2
    d = tr - g
    phi = (w * d * d - tb['c'] * tr).sum(axis=2)
    nsum = (tb['goal_mask'] * d * d).sum(axis=2)
    has_goal = r2 > 0 and variant != 'cost'
    near = (nsum <= r2) & has_goal
    viol = ((tr < tb['lo']) | (tr > tb['hi'])).any(axis=2)
    u = (tb['rho'] * act * act).sum(axis=2)[np.arange(rows) % N]
    ap = np.zeros(A) if prev_action is None else np.asarray(prev_action, np.float64)
    before = np.concatenate([np.broadcast_to(ap, (N, 1, A)), act[:, :-1]], axis=1)
    v = (tb['action_rate'] * (act - before) ** 2).sum(axis=2)[np.arange(rows) % N]
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
        r = -phi[:, t + 1] - u[:, t] - v[:, t] + np.where(ga, float(task.reward_goal), 0.0)
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


# ---------------------------------------------------------------------------------------------------------------------------------
# The closed loop: task_cases' double integrator follows pos = 0.3 sin(2 pi k / 40) from rest at the origin.  The velocity row is the one
# the integrator needs to move from one position row to the next, (pos[k + 1] - pos[k]) / DT; at most 0.471, inside the box of 1.0.
# ---------------------------------------------------------------------------------------------------------------------------------
TRACK = dict(N=64, H=10, I=3, k=8, P=2, E=2, steps=80, rms_from=40)
AMPLITUDE, PERIOD = 0.3, 40


def sine_reference(T=None):
    T = TRACK['steps'] + TRACK['H'] + 1 if T is None else T
    k = np.arange(T + 1, dtype=np.float64)
    pos = AMPLITUDE * np.sin(2.0 * np.pi * k / PERIOD)
    return np.stack([pos[:-1], (pos[1:] - pos[:-1]) / tc.DT], axis=1).astype(np.float32)


def sine_task(action_rate=None):
    """q = (1, 0.1), qT = 4 q, rho = 0.01, the velocity box of task_cases; kappa = 0 unless given."""
    return TrackingTask(reference=sine_reference(), q=[1.0, 0.1], terminal_weights=[4.0, 0.4], rho=0.01, lo=[-np.inf, -tc.VEL_BOX],
                        hi=[np.inf, tc.VEL_BOX], action_rate=action_rate)


def rms_position_error(states):
    """states [steps, 2]: the state every decision was made at -> the RMS of pos - reference pos over decisions rms_from .. steps - 1."""
    ref = sine_reference()
    k = np.arange(TRACK['rms_from'], TRACK['steps'])
    e = np.asarray(states, np.float64)[k, 0] - ref[k, 0].astype(np.float64)
    return float(np.sqrt(np.mean(e * e)))


# the RMS position error of not tracking at all (pos = 0 throughout): 0.3 / sqrt(2)
UNTRACKED_RMS = 0.212
# reference_closed_loop over seeds 0 .. 4, measured on the CPU (tests/test_tracking_cpu.py holds them to it): the worst RMS position
# error over decisions 40 .. 79 and the largest |vel|
REFERENCE_WORST_RMS = 0.0207
REFERENCE_WORST_SPEED = 0.530


def reference_closed_loop(seed, task=None):
    """task_cases.reference_closed_loop scored by planner.tracking_objective with the clock the policy keeps: decision k plans at
    (k, the action of decision k - 1).  -> (RMS position error, largest |vel| on the executed trajectory)."""
    from oracle import cem_oracle as o
    from ethz_safe_learning_amd.planner import tracking_objective
    c = TRACK
    task = sine_task() if task is None else task
    N, H, I, P = c['N'], c['H'], c['I'], c['P']
    cfg = o.PlanConfig(horizon=H, iterations=I, n_samples=N, n_elite=c['k'], particles=P, ensemble_size=c['E'], sampling_propagation=False,
                       scale_features=False)
    f = np.float32
    rng = np.random.default_rng(seed)
    lb, ub, mu0, sigma0 = o.sampling_params([-1.0], [1.0])
    s = np.array([0.0, 0.0], f)
    prev = np.zeros(1, f)
    states, vmax = [], 0.0
    for k in range(c['steps']):
        states.append(s.copy())
        mu = np.broadcast_to(mu0, (H, 1)).astype(f).copy()
        sigma = np.broadcast_to(sigma0, (H, 1)).astype(f).copy()
        best, best_score = np.zeros(1, f), f(-np.inf)
        for it in range(I):
            actions = o.sample_actions(mu, sigma, lb, ub, rng.standard_normal((N, H, 1)).astype(f))
            traj = np.zeros((N, H + 1, 2), f)
            traj[:, 0] = s
            for t in range(H):
                traj[:, t + 1] = tc.integrator_step(traj[:, t], actions[:, t, 0])
            ret, _ = tracking_objective(np.tile(traj, (P, 1, 1)), actions, task, 'cem', k0=k, prev_action=prev)
            scores = ret.reshape(P, N).sum(axis=0, dtype=f) / f(P)
            mu, sigma, best, best_score, _, _ = o.select_and_refit(scores, actions, mu, sigma, best, best_score, cfg)
        prev = np.array(best[:1], f)
        s = tc.integrator_step(s, best[0])
        vmax = max(vmax, abs(float(s[1])))
    return rms_position_error(np.array(states)), vmax
