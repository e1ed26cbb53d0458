"""Thin Python host over the C ABI: device memory and streams come from
torch-ROCm (plumbing), every computation happens in libcem_mpc_gfx950.so.

``CemPlanner`` is what the simba-shaped policies (``simba/policies``) hold; it
corresponds to one compiled ``@tf.function`` graph of the reference
(simba/policies/cem_mpc.py:35) for one set of shapes.
"""
from __future__ import annotations

import ctypes as C
import hashlib
import math
from dataclasses import dataclass, field, replace as _dc_replace
from typing import List, NamedTuple, Optional, Sequence, Tuple

import numpy as np

from . import _capi


@dataclass
class ScorerConfig:
    """SafetyGymStateScorer fields for the 'goal' task
    (reference simba/environment_utils/safety_gym.py:104-176)."""
    goal_slice: Tuple[int, int]
    observe_goal_lidar: bool = True
    lidar_max_dist: float = 4.0
    goal_size: float = 0.3
    reward_distance: float = 1.0
    reward_goal: float = 1.0
    reward_clip: float = 10.0
    constrain_indicator: bool = True
    cost_kinds: List[Tuple[int, int, float]] = field(default_factory=list)   # (lo, hi, size), reference order


def _task_table(v, n, name):
    """A task's table as float32 [n]: an array of that length, or a scalar broadcast to it."""
    a = np.asarray(v, np.float32)
    if a.ndim > 1 or (a.ndim == 1 and a.shape[0] != int(n)):
        raise ValueError('%s must be a scalar or have shape [%d]' % (name, n))
    return np.ascontiguousarray(np.broadcast_to(a, (int(n),)), dtype=np.float32)


@dataclass
class StateZones:
    """Keep-out (or keep-in) zones on a task (cem_task_zones_t; cem_mpc.h "Zones"): up to 16 axis-aligned ellipsoids on up to 4 state
    features each.  Zone z measures dist2 = sum_d weights[z, d] (s[axes[z, d]] - centre[z, d])^2 over its used axes (-1: unused).
        keep-out: a state with dist2 <= radius^2 is a violation (a cost, as a state outside the box); the reward pays
                  penalty * max((radius + margin)^2 - dist2, 0)
        keep-in:  a state with dist2 > radius^2 is a violation; the reward pays penalty * max(dist2 - (radius - margin)^2, 0)
    axes is [Z, D] (or [D]: one zone), D <= 4; centre and weights broadcast to it; radius, margin, penalty, keep_in to [Z].  Leaving
    features out makes cylinders.  Set as `zones=` of a QuadraticTask or TrackingTask."""
    axes: object = None
    centre: object = 0.0
    radius: object = 1.0
    weights: object = 1.0
    margin: object = 0.0
    penalty: object = 0.0
    keep_in: object = False

    @classmethod
    def discs(cls, features, centres, radii, margin=0.0, penalty=0.0, keep_in=False):
        """Discs (spheres) on the same `features` (say, the x and y of the state): centres [Z, len(features)], radii [Z] or one for all."""
        c = np.atleast_2d(np.asarray(centres, np.float32))
        feats = np.asarray(features, np.int64).reshape(-1)
        if c.shape[1] != feats.shape[0]:
            raise ValueError('centres must be [Z, %d]' % feats.shape[0])
        return cls(axes=np.broadcast_to(feats, c.shape).copy(), centre=c, radius=radii, margin=margin, penalty=penalty, keep_in=keep_in)

    def tables(self, obs_dim):
        """The tables as the library takes them, validated as it validates them: axis [Z, 4] int32, centre and weight [Z, 4] float32
        (zero in unused slots), radius, margin, penalty [Z] float32, keep_in [Z] int32."""
        K, ZMAX = _capi.CEM_TASK_ZONE_AXES, _capi.CEM_TASK_MAX_ZONES
        ax = np.asarray(self.axes if self.axes is not None else (), np.int64)
        if ax.ndim == 1:
            ax = ax[None]
        if ax.ndim != 2 or not 1 <= ax.shape[0] <= ZMAX or not 1 <= ax.shape[1] <= K:
            raise ValueError('axes must be [Z, D] with 1 <= Z <= %d and 1 <= D <= %d' % (ZMAX, K))
        Z, D = ax.shape
        if (ax < -1).any() or (ax >= int(obs_dim)).any():
            raise ValueError('an axis must be -1 or a feature below %d' % int(obs_dim))
        if (ax < 0).all(axis=1).any():
            raise ValueError('every zone needs a used axis')

        def per_axis(v, name):
            try:
                a = np.broadcast_to(np.asarray(v, np.float32), (Z, D))
            except ValueError:
                raise ValueError('%s must broadcast to [%d, %d]' % (name, Z, D)) from None
            out = np.zeros((Z, K), np.float32)
            out[:, :D] = np.where(ax >= 0, a, np.float32(0))
            return out

        def per_zone(v, name, dtype=np.float32):
            try:
                return np.ascontiguousarray(np.broadcast_to(np.asarray(v, dtype), (Z,)), dtype=dtype)
            except ValueError:
                raise ValueError('%s must be a scalar or have shape [%d]' % (name, Z)) from None
        axis = np.full((Z, K), -1, np.int32)
        axis[:, :D] = ax
        out = {'axis': axis, 'centre': per_axis(self.centre, 'centre'), 'weight': per_axis(self.weights, 'weights'),
               'radius': per_zone(self.radius, 'radius'), 'margin': per_zone(self.margin, 'margin'), 'penalty': per_zone(self.penalty, 'penalty')}
        kin = np.asarray(self.keep_in)
        if kin.dtype != np.bool_ and not np.isin(kin, (0, 1)).all():
            raise ValueError('keep_in must be 0 / 1')
        out['keep_in'] = per_zone(kin.astype(np.int32), 'keep_in', np.int32)
        for k in ('centre', 'weight', 'radius', 'margin', 'penalty'):
            if not np.isfinite(out[k]).all():
                raise ValueError('%s must be finite' % k)
        if (out['weight'] < 0).any() or (out['margin'] < 0).any() or (out['penalty'] < 0).any():
            raise ValueError('weights, margin and penalty must be >= 0')
        if (out['radius'] <= 0).any():
            raise ValueError('radius must be > 0')
        if ((out['keep_in'] != 0) & (out['margin'] > out['radius'])).any():
            raise ValueError('a keep-in zone needs margin <= radius')
        with np.errstate(all='ignore'):
            reach = np.where(out['keep_in'] != 0, out['radius'] - out['margin'], out['radius'] + out['margin'])
            if not (np.isfinite(out['radius'] * out['radius']).all() and np.isfinite(reach * reach).all()):
                raise ValueError('radius and margin are too large')
        return out


def _zone_tables(task, obs_dim):
    z = getattr(task, 'zones', None)
    ot = _output_tables(task, obs_dim)                # (an axis may name an output: index obs_dim + m)
    if z is None:
        return None
    if not isinstance(z, StateZones):
        raise ValueError('zones must be a StateZones')
    return z.tables(int(obs_dim) + (ot['matrix'].shape[0] if ot is not None else 0))


@dataclass
class TaskOutputs:
    """Linear outputs y = matrix @ s on a task (cem_task_outputs_t; cem_mpc.h "Linear outputs"): up to 16 derived features, each with
    the vocabulary a state feature has.  Output m pays weights[m] (y_m - target[m])^2 - linear[m] y_m (terminal_weights[m] on the last
    state of a TrackingTask), counts near[m] (y_m - target[m])^2 towards the goal radius, is a violation outside [lo[m], hi[m]], and a
    StateZones axis may name it as obs_dim + m.  matrix is [M, obs_dim] (or [obs_dim]: one output); the others are arrays of M or scalars;
    target may be [T, M] on a TrackingTask with T reference rows (the same clock).  Set as `outputs=` of a QuadraticTask or TrackingTask."""
    matrix: object = None
    weights: object = 0.0
    target: object = 0.0
    linear: object = 0.0
    near: object = 0.0
    lo: object = -np.inf
    hi: object = np.inf
    terminal_weights: object = None

    @classmethod
    def halfspaces(cls, normals, offsets):
        """The polytope normals @ s <= offsets: one output per row of `normals` [M, obs_dim], bounded above by offsets [M] (or one for all)."""
        return cls(matrix=normals, hi=offsets)

    @classmethod
    def quadratic_form(cls, Q, target, terminal=None, tol=1e-10):
        """The full-matrix cost (s - target)^T Q (s - target) as sum_i (L_i . s - L_i . target)^2: Q [obs_dim, obs_dim] symmetric positive
        semi-definite is factored in float64, Q = V diag(lam) V^T, and the rows of L are sqrt(lam_i) v_i^T for the eigenvalues above
        tol * max(lam) (an eigenvalue below -tol * max(lam) is refused; those in between are dropped).  More than 16 rows: ValueError.
        The weights are 1, the target is L @ target ([obs_dim], or [T, obs_dim] on a TrackingTask); `terminal` are terminal_weights."""
        Q = np.asarray(Q, np.float64)
        if Q.ndim != 2 or Q.shape[0] != Q.shape[1] or not np.isfinite(Q).all():
            raise ValueError('Q must be a finite square matrix')
        if not np.allclose(Q, Q.T, rtol=1e-12, atol=1e-12 * max(1.0, float(np.abs(Q).max(initial=0.0)))):
            raise ValueError('Q must be symmetric')
        lam, V = np.linalg.eigh(0.5 * (Q + Q.T))
        top = float(lam.max(initial=0.0))
        if top <= 0.0 or (lam < -float(tol) * top).any():
            raise ValueError('Q must be positive semi-definite and not zero')
        keep = lam > float(tol) * top
        if int(keep.sum()) > _capi.CEM_TASK_MAX_OUTPUTS:
            raise ValueError('the rank of Q is %d: more than %d outputs' % (int(keep.sum()), _capi.CEM_TASK_MAX_OUTPUTS))
        L = (np.sqrt(lam[keep])[:, None] * V[:, keep].T)[::-1]            # (largest eigenvalue first)
        tg = np.asarray(target, np.float64)
        if tg.ndim not in (1, 2) or tg.shape[-1] != Q.shape[0]:
            raise ValueError('target must be [%d] or [T, %d]' % (Q.shape[0], Q.shape[0]))
        return cls(matrix=L.astype(np.float32), weights=1.0, target=(tg @ L.T).astype(np.float32), terminal_weights=terminal)

    @classmethod
    def stack(cls, a, b):
        """The outputs of `a` followed by those of `b` (say, a quadratic_form and halfspaces).  A [T, M] target on one side is kept; a
        [M] target beside it is repeated over its T rows."""
        if not isinstance(a, TaskOutputs) or not isinstance(b, TaskOutputs):
            raise ValueError('stack takes two TaskOutputs')
        ma, mb = np.atleast_2d(np.asarray(a.matrix, np.float32)), np.atleast_2d(np.asarray(b.matrix, np.float32))
        if ma.shape[1] != mb.shape[1]:
            raise ValueError('the two matrices must have the same number of columns')
        ta, tb = a.tables(ma.shape[1]), b.tables(mb.shape[1])
        R = max(ta['target'].shape[0], tb['target'].shape[0])
        if {ta['target'].shape[0], tb['target'].shape[0]} - {1, R}:
            raise ValueError('the two targets have different numbers of rows')
        tg = np.concatenate([np.broadcast_to(t['target'], (R, t['target'].shape[1])) for t in (ta, tb)], axis=1)
        cat = {k: np.concatenate([ta[k], tb[k]]) for k in ('weight', 'linear', 'near', 'lo', 'hi')}
        term = None
        if ta['terminal'] is not None or tb['terminal'] is not None:
            term = np.concatenate([t['terminal'] if t['terminal'] is not None else t['weight'] for t in (ta, tb)])
        return cls(matrix=np.concatenate([ma, mb]), weights=cat['weight'], target=tg if R > 1 else tg[0], linear=cat['linear'], near=cat['near'],
                   lo=cat['lo'], hi=cat['hi'], terminal_weights=term)

    def tables(self, obs_dim, ref_rows=None):
        """The tables as the library takes them, validated as it validates them: matrix [M, obs_dim] float32, weight, linear, near, lo, hi
        [M], target [R, M] (R = 1, or the T rows of a per-step target), terminal [M] or None.  ref_rows: the base task's reference rows
        (1 for a QuadraticTask), which R must equal unless it is 1; None: not checked."""
        O, MMAX = int(obs_dim), _capi.CEM_TASK_MAX_OUTPUTS
        m = np.asarray(self.matrix if self.matrix is not None else (), np.float32)
        if m.ndim == 1 and m.shape[0] == O:
            m = m[None]
        if m.ndim != 2 or m.shape[1] != O or not 1 <= m.shape[0] <= MMAX:
            raise ValueError('matrix must be [M, %d] with 1 <= M <= %d' % (O, MMAX))
        M = m.shape[0]
        out = {'matrix': np.ascontiguousarray(m)}
        for k, v in (('weight', self.weights), ('linear', self.linear), ('near', self.near), ('lo', self.lo), ('hi', self.hi)):
            out[k] = _task_table(v, M, k)
        out['terminal'] = None if self.terminal_weights is None else _task_table(self.terminal_weights, M, 'terminal_weights')
        tg = np.asarray(self.target, np.float32)
        if tg.ndim == 2 and tg.shape[1] == M and 1 <= tg.shape[0] <= _capi.CEM_TASK_REF_MAX_STEPS:
            out['target'] = np.ascontiguousarray(tg)
        else:
            out['target'] = _task_table(tg, M, 'target')[None]
        if ref_rows is not None and out['target'].shape[0] not in (1, int(ref_rows)):
            raise ValueError('a per-step target must have the %d rows of the task\'s reference' % int(ref_rows))
        for k in ('matrix', 'weight', 'linear', 'near', 'target', 'terminal'):
            if out[k] is not None and not np.isfinite(out[k]).all():
                raise ValueError('%s must be finite' % k)
        if (out['weight'] < 0).any() or (out['terminal'] is not None and (out['terminal'] < 0).any()):
            raise ValueError('weights must be >= 0')
        if np.isnan(out['lo']).any() or np.isnan(out['hi']).any() or (out['lo'] > out['hi']).any():
            raise ValueError('the bounds must be numbers with lo <= hi')
        return out


def _output_tables(task, obs_dim):
    o = getattr(task, 'outputs', None)
    if o is None:
        return None
    if not isinstance(o, TaskOutputs):
        raise ValueError('outputs must be a TaskOutputs')
    ref = getattr(task, 'reference', None)
    return o.tables(obs_dim, ref_rows=np.asarray(ref).shape[0] if ref is not None and np.asarray(ref).ndim == 2 else 1)


@dataclass
class QuadraticTask:
    """A quadratic reward with box state constraints (cem_task_t, CEM_TASK_QUADRATIC; cem_mpc.h "Task scorers"): the objective of plans
    whose observation is no Safety-Gym lidar vector.  Per step, with s the raw state and a the action,
        reward = -sum_f [q_f (s'_f - g_f)^2 - c_f s'_f] - sum_j rho_j a_j^2 + reward_goal * near(s),   clipped to +-reward_clip (0: no clip)
        near(s) = goal_radius > 0 and sum_f goal_mask_f (s_f - g_f)^2 <= goal_radius^2             (near ends the episode, as the goal does)
        cost(s) = 1 if any s_f < lo_f or s_f > hi_f                                                  ('safe' / 'cost' handles)
    Every table is an array of the feature count or a scalar broadcast to it.  `zones` (a StateZones) adds round regions the state
    must stay out of, or inside of: a hit is a cost as leaving the box is, coming near costs reward.  `outputs` (a TaskOutputs) adds
    linear outputs y = C s with the same vocabulary: full-matrix costs, half-spaces, rotated zones."""
    q: object = 0.0
    g: object = 0.0
    c: object = 0.0
    goal_mask: object = 0.0
    lo: object = -np.inf
    hi: object = np.inf
    rho: object = 0.0
    goal_radius: float = 0.0
    reward_goal: float = 0.0
    reward_clip: float = 0.0
    outputs: object = None
    zones: object = None

    @classmethod
    def to_target(cls, target, weights=1.0, action_weights=0.0, lo=-np.inf, hi=np.inf, goal_radius=0.0, reward_goal=0.0, reward_clip=0.0, zones=None,
                  outputs=None):
        """Stay near `target`: reward = -sum weights (s - target)^2 - sum action_weights a^2; with goal_radius > 0 the episode ends (and
        reward_goal is paid) within that weighted distance of the target, measured on the features whose weight is not zero."""
        w = np.asarray(weights, np.float32)
        return cls(q=w, g=target, goal_mask=(w != 0).astype(np.float32), lo=lo, hi=hi, rho=action_weights, goal_radius=goal_radius,
                   reward_goal=reward_goal, reward_clip=reward_clip, zones=zones, outputs=outputs)

    def tables(self, obs_dim, act_dim):
        """The float32 tables as the library takes them: dict of q, g, c, goal_mask, lo, hi [obs_dim] and rho [act_dim]."""
        out = {k: _task_table(getattr(self, k), obs_dim, k) for k in ('q', 'g', 'c', 'goal_mask', 'lo', 'hi')}
        out['rho'] = _task_table(self.rho, act_dim, 'rho')
        return out

    def zone_tables(self, obs_dim):
        """StateZones.tables of `zones` (an axis may name output m as obs_dim + m), or None without zones."""
        return _zone_tables(self, obs_dim)

    def output_tables(self, obs_dim):
        """TaskOutputs.tables of `outputs`, or None without outputs."""
        return _output_tables(self, obs_dim)


@dataclass
class TrackingTask:
    """A QuadraticTask whose set-point moves with time (cem_task_tracking_t, CEM_TASK_TRACKING; cem_mpc.h "Tracking tasks"): row j of
    `reference` [T, obs_dim] takes g's place for the state that lies j - k0 steps into the plan (the last row is held), the last
    predicted state is weighted by `terminal_weights` (None: q) and every step pays sum_j action_rate_j (a_t[j] - a_{t-1}[j])^2 (None:
    nothing).  k0 and the action before the plan's first are the handle's clock (CemPlanner.set_task_clock; CemMpc keeps it).  The other
    fields are QuadraticTask's, `zones` and `outputs` among them."""
    reference: object = None
    q: object = 0.0
    c: object = 0.0
    goal_mask: object = 0.0
    lo: object = -np.inf
    hi: object = np.inf
    rho: object = 0.0
    goal_radius: float = 0.0
    reward_goal: float = 0.0
    reward_clip: float = 0.0
    terminal_weights: object = None
    action_rate: object = None
    outputs: object = None
    zones: object = None

    @classmethod
    def to_reference(cls, reference, weights=1.0, action_weights=0.0, terminal_weights=None, action_rate=None, lo=-np.inf, hi=np.inf,
                     goal_radius=0.0, reward_goal=0.0, reward_clip=0.0, zones=None, outputs=None):
        """Follow `reference` [T, obs_dim]: reward = -sum weights (s - reference row)^2 - sum action_weights a^2 - the action-rate term;
        goal_radius as QuadraticTask.to_target's, measured against the row of the moment."""
        w = np.asarray(weights, np.float32)
        return cls(reference=reference, q=w, goal_mask=(w != 0).astype(np.float32), lo=lo, hi=hi, rho=action_weights, goal_radius=goal_radius,
                   reward_goal=reward_goal, reward_clip=reward_clip, terminal_weights=terminal_weights, action_rate=action_rate, zones=zones, outputs=outputs)

    def tables(self, obs_dim, act_dim):
        """The float32 tables as the library takes them: QuadraticTask.tables' without g, q_terminal [obs_dim], action_rate [act_dim]
        and reference [T, obs_dim]."""
        O, A = int(obs_dim), int(act_dim)
        out = {k: _task_table(getattr(self, k), O, k) for k in ('q', 'c', 'goal_mask', 'lo', 'hi')}
        out['rho'] = _task_table(self.rho, A, 'rho')
        out['q_terminal'] = out['q'] if self.terminal_weights is None else _task_table(self.terminal_weights, O, 'terminal_weights')
        out['action_rate'] = _task_table(0.0 if self.action_rate is None else self.action_rate, A, 'action_rate')
        ref = np.asarray(self.reference if self.reference is not None else (), np.float32)
        if ref.ndim != 2 or ref.shape[1] != O or not 1 <= ref.shape[0] <= _capi.CEM_TASK_REF_MAX_STEPS:
            raise ValueError('reference must have shape [T, %d] with 1 <= T <= %d' % (O, _capi.CEM_TASK_REF_MAX_STEPS))
        out['reference'] = np.ascontiguousarray(ref)
        return out

    def zone_tables(self, obs_dim):
        """StateZones.tables of `zones` (an axis may name output m as obs_dim + m), or None without zones."""
        return _zone_tables(self, obs_dim)

    def output_tables(self, obs_dim):
        """TaskOutputs.tables of `outputs`, or None without outputs."""
        return _output_tables(self, obs_dim)


@dataclass
class PlannerConfig:
    """CemMpc/SafeCemMpc ctor kwargs (cem_mpc.py:7-17, safe_cem_mpc.py:8-19) +
    model dims (config/models.yaml) + sharding."""
    obs_dim: int
    act_dim: int
    ensemble_size: int
    particles: int
    n_samples: int
    horizon: int
    n_elite: int
    iterations: int
    scorer: ScorerConfig
    act_low: Sequence[float]
    act_high: Sequence[float]
    units: int = 128
    n_layers: int = 4
    activation: str = 'relu'           # mlp_params['activation'] (config/models.yaml:12): relu | tanh | sigmoid | elu | leaky_relu | softplus | selu | swish | gelu (see ACTIVATIONS)
    smoothing: float = 0.0
    stddev_threshold: float = -1.0
    noise_stddev: float = 0.0
    variant: str = 'cem'               # 'cem' | 'safe' | 'cost' (enum cem_variant; 'cost': scores = -mean cost, SafeCemMpc.optimize_for_safety)
    posterior_mean_threashold: float = 0.15
    sampling_propagation: bool = True
    scale_features: bool = True
    world_size: int = 1
    rank: int = 0
    chunks_per_tile: int = 0
    use_graph: bool = False
    rollout_segments: int = 0          # 0 auto, 1 off, n > 1: horizon-segment work queue (cem_mpc.h)
    precision: str = 'fp32'            # 'fp32' | 'bf16x3' (exact three-way bf16 split products: fp32-grade) | 'bf16' (REDUCED precision: the
                                       # operands of every dense stage rounded to bf16 once, bf16_reference_forward) — enum cem_precision, opt-in
    select_mode: int = 0               # 0 auto, 1 one-workgroup select, 2 multi-workgroup chain, 3 the chain fused into one launch (cem_mpc.h)
    constraint: str = 'beta'           # 'beta': the reference's Beta filter | 'budget': return within a cost budget (cem_planner_set_constraint,
                                       # CEM_CONSTRAINT_BUDGET; 'safe' handles only); not in cem_config_t: set after create.  The budget VALUE is
                                       # handle state (CemPlanner.set_cost_budget, default +inf), not configuration
    worst_cost_particles: int = 0      # 'budget': 0 (or particles) = the particle mean of the cumulative cost; m_c in 1 .. particles - 1: the mean
                                       # of the m_c largest particle costs (CVaR at level m_c / particles)
    refit: str = 'uniform'             # 'uniform': every elite counts 1 / k (the reference) | 'softmax': elite j counts exp((s_j - s_max) / temperature)
                                       # (cem_planner_set_refit, CEM_REFIT_SOFTMAX; n_elite = n_samples is MPPI); not in cem_config_t: set after create
    refit_temperature: float = 0.0     # 'softmax': the temperature, finite and > 0 ('uniform' ignores it)
    population: tuple = ()             # (): every iteration samples n_samples candidates (the reference); a tuple of `iterations` sizes: iteration
                                       # `it` samples population[it] (population_schedule; cem_planner_set_population_schedule); not in
                                       # cem_config_t: set after create
    mean_candidate: bool = False       # True: the last candidate of the last iteration is the clipped mean (cem_planner_set_mean_candidate)
    plan_readout: bool = False         # True: a tracker kernel behind every select keeps the best-so-far candidate's whole sequence, its particle
                                       # returns and per-step cost counts (cem_planner_set_plan_readout; CemPlanner.plan_readout); not in
                                       # cem_config_t: set after create
    task: Optional[object] = None      # None: the Safety-Gym scorer (the reference); a QuadraticTask: rollouts are scored by it
                                       # (cem_planner_set_task) and `scorer` is inert; a TrackingTask: by a reference that
                                       # moves with the handle's clock (cem_planner_set_task_tracking); either with
                                       # `zones`, a StateZones (cem_planner_set_task_zones) and `outputs`, a TaskOutputs
                                       # (cem_planner_set_task_outputs); not in cem_config_t: set after create
    action_noise: str = 'white'        # 'white': every step of a sequence drawn independently (the reference) | 'powerlaw' | 'ar1': time-correlated
                                       # noise eps = M xi with M = powerlaw_mixing / ar1_mixing(horizon, action_noise_param)
                                       # (cem_planner_set_action_noise, CEM_NOISE_MIXED); not in cem_config_t: set after create
    action_noise_param: float = 0.0    # 'powerlaw': the spectral exponent beta >= 0; 'ar1': the lag-1 correlation rho in (-1, 1); 'white' ignores it
    keep_elites: int = 0               # 0: every iteration resamples all candidates (the reference); m in 1 .. n_elite: the best m elites of an
                                       # iteration are candidates 0 .. m - 1 of the next (cem_planner_set_elite_carry); not in cem_config_t: set after create
    shift_elites: bool = False         # with keep_elites: a plan's first iteration takes the previous plan's last kept elites, shifted by elite_shift
    elite_shift: int = 1               # steps executed between two plans (shift_elites only)
    worst_particles: int = 0           # 0: score = the particle mean (the reference); m in 1 .. particles: the mean of the m smallest particle
                                       # returns (cem_planner_set_particle_objective, CEM_PARTICLES_LOWER_TAIL); not in cem_config_t: set after create


# mlp_params['activation'] is a string the reference `eval`s (mlp_ensemble.py:14): the TensorFlow names that map onto enum cem_activation
ACTIVATIONS = {'relu': 0, 'tanh': 1, 'sigmoid': 2, 'elu': 3, 'leaky_relu': 4, 'softplus': 5, 'selu': 6, 'swish': 7, 'silu': 7, 'gelu': 8}


VARIANTS = {'cem': _capi.CEM_VARIANT_CEM, 'safe': _capi.CEM_VARIANT_SAFE, 'cost': _capi.CEM_VARIANT_COST}
PARTICLE_OBJECTIVES = {'mean': _capi.CEM_PARTICLES_MEAN, 'lower_tail': _capi.CEM_PARTICLES_LOWER_TAIL}
CONSTRAINTS = {'beta': _capi.CEM_CONSTRAINT_BETA, 'budget': _capi.CEM_CONSTRAINT_BUDGET}
REFITS = {'uniform': _capi.CEM_REFIT_UNIFORM, 'softmax': _capi.CEM_REFIT_SOFTMAX}
ACTION_NOISES = ('white', 'powerlaw', 'ar1')
PRECISIONS = {'fp32': 0, 'bf16x3': 1, 'bf16': 2}   # enum cem_precision
INFEASIBLE_BELOW = np.float32(-2.0 ** 100)          # cem_mpc.h CEM_INFEASIBLE_BELOW: a constrained score is feasible iff it lies above


def rn_bf16(x) -> np.ndarray:
    """x (taken as float32) rounded to bf16 — 8 significand bits, round to nearest, ties to even — and returned as float32: bit for bit
    what the library does to a weight when it packs a precision='bf16' image (cem_rn_bf16_bits) and what v_cvt_pk_bf16_f32 does to an
    activation on the device.  Finite inputs below the largest bf16 (3.39e38); signed zeros and denormals keep their sign and round like
    every other value."""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    r = (u + np.uint64(0x7FFF) + ((u >> np.uint64(16)) & np.uint64(1))) & np.uint64(0xFFFF0000)
    return r.astype(np.uint32).view(np.float32).reshape(np.shape(x))


def bf16_reference_forward(x, member_weights):
    """The arithmetic contract of precision='bf16' for one ensemble member, in NumPy with float64 accumulation: (mu, var) of the rows x
    [B, obs + act] (the SCALED network input), `member_weights` = dict(W=[...], b=[...], W_mu, b_mu, W_var, b_var) in Keras layout
    [in, out].  Weights and the input of every dense stage — x itself and every post-ReLU activation, taken as float32 — are rounded
    with rn_bf16; products and sums are exact / float64 from the float32 bias; a stage's output is rounded to float32 (the device's
    accumulator) before the ReLU.  Softplus + 1e-4 is float32, as everywhere.  Returns arrays of x's dtype.  The device differs from
    this by the order of its float32 sums alone."""
    dt = np.asarray(x).dtype
    def dense(h, W, b):
        return (rn_bf16(h).astype(np.float64) @ rn_bf16(W).astype(np.float64) + np.asarray(b, np.float32).astype(np.float64)).astype(np.float32)
    h = np.asarray(x, np.float32)
    for W, b in zip(member_weights['W'], member_weights['b']):
        h = np.maximum(dense(h, W, b), np.float32(0))
    mu = dense(h, member_weights['W_mu'], member_weights['b_mu'])
    z = dense(h, member_weights['W_var'], member_weights['b_var'])
    # tf.math.softplus in float32 (threshold log(eps) + 2), + 1e-4
    thr = np.float32(np.log(np.finfo(np.float32).eps) + 2.0)
    with np.errstate(over='ignore'):
        ez = np.exp(z)
    var = np.where(z > -thr, z, np.where(z < thr, ez, np.log1p(ez))).astype(np.float32) + np.float32(1e-4)
    return mu.astype(dt), var.astype(dt)


def powerlaw_mixing(H, beta, dtype=np.float32) -> np.ndarray:
    """The mixing matrix M [H, H] of power-law ("coloured") action noise, eps = M xi: stationary Gaussian noise along the horizon whose
    power spectrum falls like f^-beta (beta 0 white, 1 pink, 2 red — the larger, the longer a sequence holds its direction).
        k' = min(k, H - k),  f_k = k' / H,  f_0 := 1 / H                  the folded frequency of bin k; the DC bin takes the lowest one
        lambda_k = f_k^-beta, scaled so that sum lambda = H
        m = real(ifft(sqrt(lambda))),  M[t][u] = m[(t - u) mod H]
    M is a symmetric circulant with unit rows (diag(M M^T) = 1: every step keeps unit variance, so sigma means what it meant); its
    covariance M M^T is the circulant with spectrum lambda.  beta = 0 is the identity exactly.  Like the FFT sampler of iCEM (Pinneri et
    al. 2020), which draws in the frequency domain, the correlation is PERIODIC in the horizon: step H - 1 is as correlated with step 0
    as step 1 is.  ar1_mixing has no wrap-around.  Computed in float64, returned as `dtype` (the library takes float32)."""
    H, beta = int(H), float(beta)
    if H < 1:
        raise ValueError('H must be >= 1')
    if not (math.isfinite(beta) and beta >= 0.0):
        raise ValueError('beta must be finite and >= 0, got %r' % (beta,))
    if beta == 0.0:
        return np.eye(H, dtype=dtype)
    k = np.arange(H)
    f = np.minimum(k, H - k).astype(np.float64) / H
    f[0] = 1.0 / H
    lam = f ** (-beta)
    lam *= H / lam.sum()
    m = np.real(np.fft.ifft(np.sqrt(lam)))
    t = np.arange(H)
    return np.ascontiguousarray(m[(t[:, None] - t[None, :]) % H]).astype(dtype)


def ar1_mixing(H, rho, dtype=np.float32) -> np.ndarray:
    """The mixing matrix M [H, H] of first-order autoregressive action noise, eps[t] = rho eps[t - 1] + sqrt(1 - rho^2) xi[t], eps[0] = xi[0]:
        M[t][0] = rho^t,   M[t][u] = sqrt(1 - rho^2) rho^(t - u) for 1 <= u <= t,   0 above the diagonal.
    Unit variance at every step, covariance rho^|t - t'|, no wrap-around (lower triangular: step t mixes steps 0 .. t only).  rho = 0 is
    the identity.  Computed in float64, returned as `dtype`."""
    H, rho = int(H), float(rho)
    if H < 1:
        raise ValueError('H must be >= 1')
    if not -1.0 < rho < 1.0:                        # (NaN fails both comparisons)
        raise ValueError('rho must lie in (-1, 1), got %r' % (rho,))
    t = np.arange(H)
    lag = t[:, None] - t[None, :]
    M = np.where(lag >= 0, rho ** np.maximum(lag, 0).astype(np.float64), 0.0)
    M[:, 1:] *= math.sqrt(1.0 - rho * rho)
    return np.ascontiguousarray(M).astype(dtype)


def mix_noise(M, xi) -> np.ndarray:
    """Host restatement of CEM_NOISE_MIXED (cem_mpc.h), bit for bit: xi [..., H, A] white normals (CemPlanner.fill_noise's eps_act) ->
    eps [..., H, A] with eps[..., t, a] = the fp32 sum over u = 0 .. H - 1, in that order and starting from +0, of fl32(M[t][u] * xi[..., u, a]).
    The product and the sum are separate float32 operations, as on the device."""
    M = np.asarray(M, np.float32)
    x = np.asarray(xi, np.float32)
    H = M.shape[0]
    if M.shape != (H, H) or x.ndim < 2 or x.shape[-2] != H:
        raise ValueError('M must be [H, H] and xi [..., H, A]')
    acc = np.zeros(x.shape, np.float32)
    for u in range(H):
        acc = acc + M[:, u][:, None] * x[..., u, :][..., None, :]
    return acc


def mixing_matrix(kind, param, H):
    """None for 'white', else the [H, H] float32 matrix of 'powerlaw' (param = beta) or 'ar1' (param = rho)."""
    if kind not in ACTION_NOISES:
        raise ValueError("action noise is 'white', 'powerlaw' or 'ar1', got %r" % (kind,))
    if kind == 'white':
        return None
    return powerlaw_mixing(H, param) if kind == 'powerlaw' else ar1_mixing(H, param)


def encode_infeasible(total) -> np.float32:
    """cem_f32_encode_infeasible (cem_mpc.h): the score of an infeasible candidate whose summed cost is the integer `total` in [0, 2^23):
    -(float)(2^23 + total) * 2^77, exact in fp32 and strictly decreasing in total.  Arrays in, arrays out."""
    t = np.asarray(total, np.int64)
    if ((t < 0) | (t >= 1 << 23)).any():
        raise ValueError('total must lie in [0, 2^23)')
    return -((t + (1 << 23)).astype(np.float32)) * np.float32(2.0 ** 77)


def decode_constrained_score(score):
    """(feasible, total_or_None) of one score of a 'budget' handle (cem_f32_score_is_feasible / cem_f32_decode_infeasible): feasible iff
    score > -2^100, and then the score is the mean return; otherwise total = -score * 2^-77 - 2^23, the integer cost that ranked it."""
    s = np.float32(score)
    if s > INFEASIBLE_BELOW:
        return True, None
    return False, int(-s * np.float32(2.0 ** -77)) - (1 << 23)


def risk_particles(risk_level, particles) -> int:
    """The m of the lower-tail particle objective for a CVaR level: m = min(P, max(1, ceil(risk_level * P - 1e-9))), risk_level in (0, 1].
    (The guard: 0.07 * 100 is 7.000000000000001 in float64 and would round up to 8.)"""
    level, P = float(risk_level), int(particles)
    if not 0.0 < level <= 1.0:                      # (NaN fails both comparisons)
        raise ValueError('risk_level must lie in (0, 1], got %r' % (risk_level,))
    if P < 1:
        raise ValueError('particles must be >= 1')
    return min(P, max(1, int(math.ceil(level * P - 1e-9))))


def activation_code(name) -> int:
    """'tf.nn.relu' / 'tf.nn.tanh' / 'tf.math.tanh' / 'tf.keras.activations.elu' / 'tf.nn.swish' / 'relu' ... -> enum cem_activation.  Raises
    for anything else.  (swish / silu and gelu are not monotone — their derivative is not a function of the layer's output — so the
    device trainer keeps the pre-activations of those layers; gelu is TensorFlow's default exact form, approximate=False.)"""
    key = str(name).strip().split('.')[-1].lower()
    if key not in ACTIVATIONS:
        raise NotImplementedError("activation %r is not built (supported: %s — as bare names or with a tf.nn. / tf.math. / "
                                  "tf.keras.activations. prefix)" % (name, ', '.join(sorted(ACTIVATIONS))))
    return ACTIVATIONS[key]


def sampling_params(low, high):
    """MpcPolicy.sampling_params (reference simba/policies/mpc_policy.py:45-57)."""
    low = np.asarray(low, np.float32)
    high = np.asarray(high, np.float32)
    if np.all(np.isfinite(low)) and np.all(np.isfinite(high)):
        return low, high, (high + low) / np.float32(2.0), (high - low) / np.float32(2.0)
    a = low.shape[0]
    return (np.full(a, -100, np.float32), np.full(a, 100, np.float32), np.zeros(a, np.float32),
            np.full(a, 100, np.float32))


def to_c_config(cfg: PlannerConfig) -> _capi.CemConfig:
    c = _capi.CemConfig()
    c.abi_version = _capi.CEM_ABI_VERSION
    c.obs_dim, c.act_dim, c.units, c.n_layers = cfg.obs_dim, cfg.act_dim, cfg.units, cfg.n_layers
    c.activation = activation_code(cfg.activation)
    c.ensemble_size, c.particles, c.n_samples = cfg.ensemble_size, cfg.particles, cfg.n_samples
    c.horizon, c.n_elite, c.iterations = cfg.horizon, cfg.n_elite, cfg.iterations
    c.smoothing, c.stddev_threshold, c.noise_stddev = cfg.smoothing, cfg.stddev_threshold, cfg.noise_stddev
    # `(1.0 - self.smoothing)` is a Python-float difference that TF converts once to fp32 (cem_mpc.py:64-65)
    c.one_minus_smoothing = float(np.float32(1.0 - float(cfg.smoothing)))
    if cfg.variant not in VARIANTS:
        raise ValueError("variant must be 'cem', 'safe' or 'cost'")
    c.variant = VARIANTS[cfg.variant]
    c.posterior_mean_threashold = cfg.posterior_mean_threashold
    c.sampling_propagation = int(bool(cfg.sampling_propagation))
    c.scale_features = int(bool(cfg.scale_features))
    if cfg.act_dim > _capi.CEM_MAX_ACT:
        raise ValueError('act_dim > %d' % _capi.CEM_MAX_ACT)
    lb, ub, mu0, sg0 = sampling_params(cfg.act_low, cfg.act_high)
    if lb.shape != (cfg.act_dim,):
        raise ValueError('act_low/act_high must have shape [act_dim]')
    for a in range(cfg.act_dim):
        c.act_lb[a], c.act_ub[a], c.act_mu0[a], c.act_sigma0[a] = float(lb[a]), float(ub[a]), float(mu0[a]), float(sg0[a])
    s = cfg.scorer
    c.scorer.goal_mode = 0 if s.observe_goal_lidar else 1
    c.scorer.goal_lo, c.scorer.goal_hi = int(s.goal_slice[0]), int(s.goal_slice[1])
    c.scorer.lidar_max_dist, c.scorer.goal_size = s.lidar_max_dist, s.goal_size
    # goal_achieved = dist <= self.goal_size * 0.8 (safety_gym.py:116): a Python-float product converted to an fp32 tensor
    c.scorer.goal_reached_dist = float(np.float32(float(s.goal_size) * 0.8))
    c.scorer.reward_distance, c.scorer.reward_goal = s.reward_distance, s.reward_goal
    c.scorer.reward_clip = float(s.reward_clip) if s.reward_clip else 0.0
    c.scorer.constrain_indicator = int(bool(s.constrain_indicator))
    if len(s.cost_kinds) > _capi.CEM_MAX_COST_KINDS:
        raise ValueError('too many cost kinds')
    c.scorer.n_cost_kinds = len(s.cost_kinds)
    for i, (lo, hi, size) in enumerate(s.cost_kinds):
        c.scorer.cost_lo[i], c.scorer.cost_hi[i], c.scorer.cost_size[i] = int(lo), int(hi), float(size)
    c.world_size, c.rank, c.chunks_per_tile, c.use_graph = cfg.world_size, cfg.rank, cfg.chunks_per_tile, int(cfg.use_graph)
    c.rollout_segments = int(cfg.rollout_segments)
    c.precision = PRECISIONS[cfg.precision]
    c.select_mode = int(cfg.select_mode)
    return c


def flatten_weights(weights) -> np.ndarray:
    """Keras-layout per-member weights -> the natural blob of cem_mpc.h:
    W_0,b_0,...,W_{L-1},b_{L-1},W_mu,b_mu,W_var,b_var per member, [in][out] row-major."""
    parts = []
    for w in weights:
        for W, b in zip(w['W'], w['b']):
            parts += [np.asarray(W, np.float32).ravel(), np.asarray(b, np.float32).ravel()]
        parts += [np.asarray(w['W_mu'], np.float32).ravel(), np.asarray(w['b_mu'], np.float32).ravel(),
                  np.asarray(w['W_var'], np.float32).ravel(), np.asarray(w['b_var'], np.float32).ravel()]
    return np.ascontiguousarray(np.concatenate(parts))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _np_ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None else None


class CemPlanner:
    """One planner handle (fixed shapes) on one GPU."""

    max_batch = 1                                     # problems (= carry slots) of the handle; BatchCemPlanner sets its own

    def __init__(self, cfg: PlannerConfig, device='cuda:0'):
        import torch
        self._torch = torch
        self.lib = _capi.load()                       # raises if the HIP extension is missing
        if not torch.cuda.is_available():
            raise RuntimeError('%s needs a ROCm GPU (torch.cuda.is_available() is False); there is no CPU path' % type(self).__name__)
        self.cfg = cfg
        self.ccfg = to_c_config(cfg)
        self.device = torch.device(device)
        nbytes = self._workspace_bytes()
        if nbytes == 0:
            # let create() report the precise status
            nbytes = 256
        with torch.cuda.device(self.device):
            self.workspace = torch.zeros(nbytes + 256, dtype=torch.uint8, device=self.device)
            off = (-self.workspace.data_ptr()) % 256
            self._ws_view = self.workspace[off:off + nbytes]
            # a stream of the planner's own: the legacy default stream cannot be captured into a hipGraph
            self.stream = torch.cuda.Stream(device=self.device)
            torch.cuda.synchronize(self.device)         # workspace zero-fill (default stream) before the library uses it
            h = C.c_void_p()
            self._create(_ptr(self._ws_view), nbytes, C.c_void_p(self.stream.cuda_stream), C.byref(h))
        self.h = h
        lay = _capi.CemLayout()
        _capi.check(self.lib.cem_planner_layout(self.h, C.byref(lay)), 'cem_planner_layout')
        self.layout = lay
        self._call = 0
        self.has_comm = False
        self.task = None                              # the QuadraticTask or TrackingTask in force (set_task)
        self.task_clock = None                        # a TrackingTask's clock as last set: (k0, previous action [A]) (set_task_clock)
        # the configured options, in this order: (is it configured?, the call that applies it).  A handle that refuses one is closed
        options = (
            (cfg.worst_particles, lambda: self.set_particle_objective('lower_tail', cfg.worst_particles)),
            (cfg.constraint != 'beta' or cfg.worst_cost_particles, lambda: self.set_constraint(cfg.constraint, cfg.worst_cost_particles)),
            (cfg.refit != 'uniform', lambda: self.set_refit(cfg.refit, cfg.refit_temperature)),
            (cfg.action_noise != 'white', lambda: self.set_action_noise(cfg.action_noise, cfg.action_noise_param)),
            (cfg.keep_elites, lambda: self.set_elite_carry(cfg.keep_elites, cfg.shift_elites, cfg.elite_shift)),
            (cfg.population, lambda: self.set_population_schedule(cfg.population)),
            (cfg.mean_candidate, lambda: self.set_mean_candidate(True)),
            (cfg.plan_readout, lambda: self.set_plan_readout(True)),
            (cfg.task is not None, lambda: self.set_task(cfg.task)),
        )
        try:
            for configured, apply in options:
                if configured:
                    apply()
        except Exception:
            self.close()
            raise
        self.have_device_weights = False              # the last weight sync came from device memory (set_weights_dev / set_weights_from)
        # the generate_action hot path: staging buffers and their ctypes views are made once (a.ctypes.data_as and the two small
        # numpy allocations were 12 of the 17 us the wrapper added to a 1.9-ms plan)
        self._st_buf = np.zeros(cfg.obs_dim, np.float32)
        self._act_buf = np.zeros(cfg.act_dim, np.float32)
        self._st_ptr, self._act_ptr = _np_ptr(self._st_buf), _np_ptr(self._act_buf)
        self._score, self._iters = C.c_float(), C.c_int32()
        self._score_ref, self._iters_ref = C.byref(self._score), C.byref(self._iters)

    # the two library calls a batch handle makes differently (BatchCemPlanner)
    def _workspace_bytes(self):
        return self.lib.cem_workspace_bytes(C.byref(self.ccfg))

    def _create(self, ws_ptr, nbytes, stream, out):
        _capi.check(self.lib.cem_planner_create(C.byref(self.ccfg), ws_ptr, nbytes, stream, out), 'cem_planner_create')

    # ------------------------------------------------------------------ stream plumbing
    def _wait_inputs(self):
        """Order the planner's stream after whatever torch's current stream has queued (input tensors)."""
        self.stream.wait_stream(self._torch.cuda.current_stream(self.device))

    def stream_context(self):
        """Context in which torch ops (the RCCL collective on the score buffers) run on the planner's stream."""
        return self._torch.cuda.stream(self.stream)

    def synchronize(self):
        self.stream.synchronize()

    # ------------------------------------------------------------------ views
    # Views into the workspace (no copy).  plan() may return before the planner's stream has drained — it watches the pinned result
    # block, not the stream (cem_mpc.h, cem_planner_plan) — and these arrays are written by the kernels behind that result, on a
    # stream torch's current stream knows nothing about: every accessor therefore drains the planner's stream first.  sync=False is for
    # callers that enqueue work on the planner's own stream (`with planner.stream_context():`), where stream order already holds.
    # What stays the caller's job: a view is not a copy.  A kernel the caller queues on ANOTHER stream to read one is ordered behind the
    # plan that wrote it (the drain above) but not in front of the NEXT plan, which overwrites the same bytes — the generator path of
    # plan() waits for nobody.  Finish with the view (or clone it) before the next plan call, or queue the reader on the planner's stream.
    def _view(self, off, count, dtype, sync=True):
        t = self._torch
        if sync:
            self.stream.synchronize()
        nb = count * t.tensor([], dtype=dtype).element_size()
        return self._ws_view[off:off + nb].view(dtype)

    @property
    def n_local(self):
        return self.cfg.n_samples // self.cfg.world_size

    def scores_local(self, sync=True):
        return self._view(self.layout.scores_local, self.n_local, self._torch.float32, sync)

    def scores_global(self, sync=True):
        return self._view(self.layout.scores_global, self.cfg.n_samples, self._torch.float32, sync)

    def actions(self, sync=True):
        c = self.cfg
        return self._view(self.layout.actions, c.n_samples * c.horizon * c.act_dim, self._torch.float32, sync).view(
            c.n_samples, c.horizon, c.act_dim)

    def mu_sigma(self, sync=True):
        c = self.cfg
        return self._view(self.layout.mu_sigma, 2 * c.horizon * c.act_dim, self._torch.float32, sync).view(2, c.horizon, c.act_dim)

    def elite_idx(self, sync=True):
        return self._view(self.layout.elite_idx, self.cfg.n_elite, self._torch.int32, sync)

    def returns(self, sync=True):
        c = self.cfg
        return self._view(self.layout.returns, c.particles * self.n_local, self._torch.float32, sync).view(c.particles, self.n_local)

    def costs(self, sync=True):
        c = self.cfg
        return self._view(self.layout.costs, c.horizon * c.particles * self.n_local, self._torch.uint8, sync).view(
            c.horizon, c.particles, self.n_local)

    def result_block(self, sync=True):
        """The last completed plan's result as the device keeps it (cem_layout_t.result): uint32 [38] — [0, A) action bits, [32] score
        bits, [33] iterations, [34] early-stop flag, [35] fault bits, [36] plan counter, [37] checksum."""
        return self._view(self.layout.result, 38, self._torch.int32, sync)

    # ------------------------------------------------------------------ sync hooks
    def set_weights(self, weights):
        blob = flatten_weights(weights)
        expect = self.lib.cem_weight_blob_floats(C.byref(self.ccfg))
        if blob.size != expect:
            raise ValueError('weight blob has %d floats, expected %d' % (blob.size, expect))
        _capi.check(self.lib.cem_planner_set_weights(self.h, _np_ptr(blob), blob.size), 'cem_planner_set_weights')
        self.have_device_weights = False

    def set_weights_dev(self, blob):
        """The same sync from the device (cem_planner_set_weights_dev): ``blob`` is a contiguous fp32 tensor on the planner's device
        holding the natural blob (flatten_weights' layout; CemTrainer.weights_dev() is one).  The images are packed by kernels on the
        planner's stream, which first waits for what torch's current stream has queued; nothing synchronises with the host."""
        t = self._torch
        if not (t.is_tensor(blob) and blob.is_cuda and blob.device == self.device and blob.dtype == t.float32 and blob.is_contiguous()):
            raise ValueError('set_weights_dev takes a contiguous float32 tensor on %s' % (self.device,))
        self._wait_inputs()
        _capi.check(self.lib.cem_planner_set_weights_dev(self.h, _ptr(blob), blob.numel()), 'cem_planner_set_weights_dev')
        blob.record_stream(self.stream)
        self.have_device_weights = True

    def set_weights_from(self, trainer):
        """Take a CemTrainer's current weights where they live.  Same device: the planner's stream waits on an event recorded on the
        trainer's stream and the pack kernels read the trainer's workspace; the trainer's stream in turn waits on an event recorded
        behind the pack kernels, so its next step does not overwrite the blob while they read it; no host synchronise either way.
        Another device: the host route."""
        if trainer.device != self.device:
            self.set_weights(trainer.get_weights())
            return
        t = self._torch
        blob = trainer.weights_dev()
        if trainer.stream != self.stream:
            ev = t.cuda.Event()
            ev.record(trainer.stream)
            self.stream.wait_event(ev)
        _capi.check(self.lib.cem_planner_set_weights_dev(self.h, _ptr(blob), blob.numel()), 'cem_planner_set_weights_dev')
        if trainer.stream != self.stream:
            packed = t.cuda.Event()
            packed.record(self.stream)
            trainer.stream.wait_event(packed)
        self.have_device_weights = True

    def weight_images(self):
        """The device arrays the rollout kernels read their weights from, as uint32 NumPy copies: wpack, bias_h, bias_mu, bias_var, etab
        (cem_layout_t).  Waits for the planner's stream.  For tests and debugging."""
        t, lay, c = self._torch, self.layout, self.cfg
        sizes = dict(wpack=lay.wpack_bytes, bias_h=c.ensemble_size * c.n_layers * 512, bias_mu=c.ensemble_size * 512,
                     bias_var=c.ensemble_size * 512, etab=lay.etab_bytes)
        return {k: self._view(getattr(lay, k), n // 4, t.int32).cpu().numpy().view(np.uint32) for k, n in sizes.items()}

    def set_normaliser(self, inputs_min, inputs_max):
        mn = np.ascontiguousarray(np.asarray(inputs_min, np.float32))
        mx = np.ascontiguousarray(np.asarray(inputs_max, np.float32))
        if mn.shape != (self.cfg.obs_dim + self.cfg.act_dim,) or mx.shape != mn.shape:
            raise ValueError('normaliser must have shape [obs_dim + act_dim]')
        _capi.check(self.lib.cem_planner_set_normaliser(self.h, _np_ptr(mn), _np_ptr(mx)), 'cem_planner_set_normaliser')

    # ------------------------------------------------------------------ native exchange (RCCL inside the library)
    def comm_init(self, group=None):
        """Give the handle its own RCCL communicator over the ranks of ``group`` (default: the world), so that ``plan()`` runs
        the whole candidate-sharded plan — kernels and the per-iteration all-gather of the scores — inside the library, as one
        hipGraph per rank when ``use_graph`` is set.  Collective: every rank of the group calls it.  torch.distributed only
        carries the 128-byte communicator id from rank 0 to the others; with world_size 1 it is not needed at all."""
        c = self.cfg
        buf = (C.c_char * _capi.CEM_COMM_ID_BYTES)()
        if c.world_size > 1:
            import torch.distributed as dist
            if not (dist.is_available() and dist.is_initialized()):
                raise RuntimeError('comm_init for world_size > 1 needs an initialised torch.distributed process group (it carries the id)')
            if dist.get_world_size(group) != c.world_size or dist.get_rank(group) != c.rank:
                raise ValueError('the process group does not match the planner\'s (world_size, rank)')
            box = [None]
            if c.rank == 0:
                _capi.check(self.lib.cem_comm_unique_id(buf), 'cem_comm_unique_id')
                box[0] = bytes(buf.raw)
            src = dist.get_global_rank(group, 0) if group is not None else 0
            dist.broadcast_object_list(box, src=src, group=group)
            buf.raw = box[0]
        else:
            _capi.check(self.lib.cem_comm_unique_id(buf), 'cem_comm_unique_id')
        with self._torch.cuda.device(self.device):
            _capi.check(self.lib.cem_planner_comm_init(self.h, buf, c.world_size, c.rank), 'cem_planner_comm_init')
        self.has_comm = True

    def comm_ranks(self):
        """Ranks of the handle's RCCL communicator as RCCL reports them (0 without one)."""
        n = C.c_int32()
        _capi.check(self.lib.cem_planner_comm_ranks(self.h, C.byref(n)), 'cem_planner_comm_ranks')
        return n.value

    def comm_destroy(self):
        _capi.check(self.lib.cem_planner_comm_destroy(self.h), 'cem_planner_comm_destroy')
        self.has_comm = False

    def graph_status(self):
        """'eager' | 'graph' | 'graph-unsupported' (cem_planner_graph_status)."""
        st = C.c_int32()
        _capi.check(self.lib.cem_planner_graph_status(self.h, C.byref(st)), 'cem_planner_graph_status')
        return ('eager', 'graph', 'graph-unsupported')[st.value]

    def graph_nodes(self):
        """Nodes of the captured plan as the runtime counts them (cem_planner_graph_nodes); 0 while no graph is held."""
        n = C.c_int32()
        _capi.check(self.lib.cem_planner_graph_nodes(self.h, C.byref(n)), 'cem_planner_graph_nodes')
        return n.value

    def launches_per_iteration(self):
        """Kernel launches one CEM iteration of plan() takes on this handle (cem_planner_launches_per_iteration)."""
        n = C.c_int32()
        _capi.check(self.lib.cem_planner_launches_per_iteration(self.h, C.byref(n)), 'cem_planner_launches_per_iteration')
        return n.value

    def rollout_path(self):
        """'generic' | 'lean': the rollout kernels plan() launches on this handle when it is given no noise tensors (cem_planner_rollout_path)."""
        n = C.c_int32()
        _capi.check(self.lib.cem_planner_rollout_path(self.h, C.byref(n)), 'cem_planner_rollout_path')
        return ('generic', 'lean')[n.value]

    def rollout_form(self, it=0):
        """0 generic | 1 lean, branchy form | 2 lean, straight-line form: what iteration `it` launches (cem_planner_rollout_form)."""
        n = C.c_int32()
        _capi.check(self.lib.cem_planner_rollout_form(self.h, int(it), C.byref(n)), 'cem_planner_rollout_form')
        return n.value

    def set_particle_objective(self, kind='mean', m=0):
        """How a candidate's particle returns become its score (cem_planner_set_particle_objective): 'mean' (the reference, the default)
        or 'lower_tail' with m in 1 .. particles, the mean of the m smallest returns.  Sticky; a change re-captures the graph."""
        if kind not in PARTICLE_OBJECTIVES:
            raise ValueError("kind is 'mean' or 'lower_tail'")
        _capi.check(self.lib.cem_planner_set_particle_objective(self.h, PARTICLE_OBJECTIVES[kind], int(m)), 'cem_planner_set_particle_objective')

    def particle_objective(self):
        """('mean', 0) or ('lower_tail', m) (cem_planner_get_particle_objective)."""
        kind, m = C.c_int32(), C.c_int32()
        _capi.check(self.lib.cem_planner_get_particle_objective(self.h, C.byref(kind), C.byref(m)), 'cem_planner_get_particle_objective')
        return ('mean', 'lower_tail')[kind.value], m.value

    def set_constraint(self, kind='beta', worst_cost_particles=0):
        """What a 'safe' handle's cost bytes do to the scores (cem_planner_set_constraint): 'beta' (the reference's filter, the default) or
        'budget' — return within the cost budget of set_cost_budget, on the particle mean of the cumulative cost (worst_cost_particles 0)
        or on the mean of its m_c largest particles.  Sticky; a change re-captures the graph."""
        if kind not in CONSTRAINTS:
            raise ValueError("kind is 'beta' or 'budget'")
        _capi.check(self.lib.cem_planner_set_constraint(self.h, CONSTRAINTS[kind], int(worst_cost_particles)), 'cem_planner_set_constraint')

    def constraint(self):
        """('beta', 0) or ('budget', m_c), m_c = particles for the mean form (cem_planner_get_constraint)."""
        kind, m = C.c_int32(), C.c_int32()
        _capi.check(self.lib.cem_planner_get_constraint(self.h, C.byref(kind), C.byref(m)), 'cem_planner_get_constraint')
        return ('beta', 'budget')[kind.value], m.value

    def set_cost_budget(self, budget):
        """The budget(s) of the 'budget' constraint: a scalar sets every problem row of the handle, an array rows 0 .. n - 1 of a batch
        handle.  A stream-ordered copy: later plans see it, the captured graph stays (cem_planner_set_cost_budget).  Default +inf."""
        b = np.ascontiguousarray(np.asarray(budget, np.float32).reshape(-1))
        self.budget_staged = None                     # (whatever a policy noted about the handle's budget no longer holds: SafeCemMpc._stage_budget)
        _capi.check(self.lib.cem_planner_set_cost_budget(self.h, _np_ptr(b), b.size), 'cem_planner_set_cost_budget')

    def constraint_costs(self, problem=0, n=None):
        """The cost statistic C [n] of every candidate of `problem` as the last constrained reduce left it (cem_planner_constraint_costs);
        n defaults to the handle's candidates.  Waits for the planner's stream."""
        out = np.zeros(self.n_local if n is None else int(n), np.float32)
        _capi.check(self.lib.cem_planner_constraint_costs(self.h, int(problem), _np_ptr(out), out.size), 'cem_planner_constraint_costs')
        return out

    def set_refit(self, kind='uniform', temperature=0.0):
        """What an iteration does with the elites' scores (cem_planner_set_refit): 'uniform' (the reference's 1 / k, the default) or
        'softmax' — elite j counts exp((s_j - s_max) / temperature) in the mean and the variance (MPPI when n_elite = n_samples).
        Sticky; a change, of the temperature alone too, re-captures the graph."""
        if kind not in REFITS:
            raise ValueError("kind is 'uniform' or 'softmax'")
        _capi.check(self.lib.cem_planner_set_refit(self.h, REFITS[kind], float(temperature)), 'cem_planner_set_refit')

    def refit(self):
        """('uniform', 0.0) or ('softmax', temperature) (cem_planner_get_refit)."""
        kind, t = C.c_int32(), C.c_float()
        _capi.check(self.lib.cem_planner_get_refit(self.h, C.byref(kind), C.byref(t)), 'cem_planner_get_refit')
        return ('uniform', 'softmax')[kind.value], t.value

    def refit_stats(self, problem=0, n=None):
        """The effective sample size W^2 / sum w^2 of iterations 0 .. n - 1 of `problem`'s last weighted plan (cem_planner_refit_stats);
        n defaults to the handle's iterations — pass the plan's `iters` after an early stop.  Waits for the planner's stream."""
        out = np.zeros(self.cfg.iterations if n is None else int(n), np.float32)
        _capi.check(self.lib.cem_planner_refit_stats(self.h, int(problem), _np_ptr(out), out.size), 'cem_planner_refit_stats')
        return out

    def set_action_noise(self, kind_or_matrix='white', param=None):
        """What the sampler multiplies by sigma (cem_planner_set_action_noise): 'white' (the reference, the default), 'powerlaw' with
        param = beta, 'ar1' with param = rho, or an [H, H] mixing matrix of the caller's own (row = output step); then eps = M xi along
        the horizon (mix_noise restates it).  Sticky; a change waits for the stream and re-captures the graph."""
        H = self.cfg.horizon
        if isinstance(kind_or_matrix, str):
            M = mixing_matrix(kind_or_matrix, 0.0 if param is None else param, H)
        else:
            M = np.ascontiguousarray(np.asarray(kind_or_matrix, np.float32))
            if M.shape != (H, H):
                raise ValueError('the mixing matrix must have shape [%d, %d]' % (H, H))
        kind = _capi.CEM_NOISE_WHITE if M is None else _capi.CEM_NOISE_MIXED
        _capi.check(self.lib.cem_planner_set_action_noise(self.h, kind, _np_ptr(M)), 'cem_planner_set_action_noise')

    def action_noise(self):
        """('white', None) or ('mixed', M [H, H]) as set (cem_planner_get_action_noise)."""
        kind = C.c_int32()
        M = np.zeros((self.cfg.horizon, self.cfg.horizon), np.float32)
        _capi.check(self.lib.cem_planner_get_action_noise(self.h, C.byref(kind), _np_ptr(M)), 'cem_planner_get_action_noise')
        return ('white', None) if kind.value == _capi.CEM_NOISE_WHITE else ('mixed', M)

    def action_noise_floats(self):
        """Floats of the handle's mixed-noise allocation (cem_planner_action_noise_dev): 0 on a handle that has never been 'mixed'."""
        ptr, n = C.c_void_p(), C.c_size_t()
        _capi.check(self.lib.cem_planner_action_noise_dev(self.h, C.byref(ptr), C.byref(n)), 'cem_planner_action_noise_dev')
        return int(n.value) if ptr.value else 0

    def action_noise_tensor(self, problem=0):
        """eps [I, N, H, A] of `problem` as the handle's last 'mixed' plan sampled from it (cem_planner_action_noise_dev), on the host.
        Waits for the planner's stream.  Raises on a handle that has never been 'mixed'."""
        c, t = self.cfg, self._torch
        ptr, n = C.c_void_p(), C.c_size_t()
        _capi.check(self.lib.cem_planner_action_noise_dev(self.h, C.byref(ptr), C.byref(n)), 'cem_planner_action_noise_dev')
        per = c.iterations * c.n_samples * c.horizon * c.act_dim
        if not ptr.value:
            raise RuntimeError('the handle has no mixed action noise (set_action_noise was never given a matrix)')
        if not 0 <= int(problem) < n.value // per:
            raise ValueError('problem out of range')

        class _Dev:                                   # the library's allocation as torch sees foreign device memory
            __cuda_array_interface__ = dict(shape=(per,), typestr='<f4', data=(ptr.value + 4 * per * int(problem), False), version=2)
        self.synchronize()
        with t.cuda.device(self.device):
            out = t.as_tensor(_Dev(), device=self.device).cpu().numpy().copy()
        return out.reshape(c.iterations, c.n_samples, c.horizon, c.act_dim)

    def set_elite_carry(self, n_keep, across_plans=False, shift=1):
        """Elite carry-over (cem_planner_set_elite_carry): the best `n_keep` elites of an iteration are candidates 0 .. n_keep - 1 of the
        next one; with across_plans also of the next plan's first iteration, moved `shift` steps towards the present (the freed tail
        keeps the sampler's draw).  0 switches it off.  keep_elites / inject_elites restate the two kernels.  Sticky; every call empties
        the stores, waits for the stream and re-captures the graph.  The store lives on the HANDLE: with across_plans two users of one
        handle would continue each other's plans (owner= of cached_planner)."""
        ec = _capi.CemEliteCarry(n_keep=int(n_keep), across_plans=int(bool(across_plans)), shift=int(shift), reserved=0)
        _capi.check(self.lib.cem_planner_set_elite_carry(self.h, C.byref(ec)), 'cem_planner_set_elite_carry')

    def elite_carry(self):
        """(n_keep, across_plans, shift) as set (cem_planner_get_elite_carry)."""
        ec = _capi.CemEliteCarry()
        _capi.check(self.lib.cem_planner_get_elite_carry(self.h, C.byref(ec)), 'cem_planner_get_elite_carry')
        return ec.n_keep, bool(ec.across_plans), ec.shift

    def elite_store(self, problem=0):
        """(E [n_keep, H, A], count) of `problem` as the stream leaves them (cem_planner_elite_store).  Waits for the planner's stream."""
        c = self.cfg
        E = np.zeros((self.elite_carry()[0], c.horizon, c.act_dim), np.float32)
        n = C.c_int32()
        _capi.check(self.lib.cem_planner_elite_store(self.h, int(problem), _np_ptr(E), C.byref(n)), 'cem_planner_elite_store')
        return E, n.value

    def set_population_schedule(self, n=None):
        """Per-iteration population sizes (cem_planner_set_population_schedule): iteration `it` samples, rolls out and ranks n[it] candidates,
        exactly as a handle created with n_samples = n[it] would.  None, or every entry equal to n_samples, switches it off.  Sticky."""
        if n is None or len(n) == 0:
            _capi.check(self.lib.cem_planner_set_population_schedule(self.h, None, 0), 'cem_planner_set_population_schedule')
            return
        arr = (C.c_int32 * len(n))(*[int(x) for x in n])
        _capi.check(self.lib.cem_planner_set_population_schedule(self.h, arr, len(n)), 'cem_planner_set_population_schedule')

    def population_schedule(self):
        """(sizes [iterations], enabled) as set (cem_planner_get_population_schedule): n_samples everywhere while off."""
        arr = (C.c_int32 * self.cfg.iterations)()
        on = C.c_int32()
        _capi.check(self.lib.cem_planner_get_population_schedule(self.h, arr, self.cfg.iterations, C.byref(on)), 'cem_planner_get_population_schedule')
        return list(arr), bool(on.value)

    def iteration_plan(self, it):
        """What iteration `it` launches (cem_planner_iteration_plan), on any handle: a dict of n_samples, chunks_per_tile, n_tiles,
        n_segments, n_pinned, launches and rollout_path ('lean' / 'generic')."""
        ip = _capi.CemIterationPlan()
        _capi.check(self.lib.cem_planner_iteration_plan(self.h, int(it), C.byref(ip)), 'cem_planner_iteration_plan')
        return dict(n_samples=ip.n_samples, chunks_per_tile=ip.chunks_per_tile, n_tiles=ip.n_tiles, n_segments=ip.n_segments,
                    n_pinned=ip.n_pinned, launches=ip.launches, rollout_path='lean' if ip.rollout_path else 'generic')

    def set_mean_candidate(self, enable=True):
        """The last candidate of the last iteration becomes the clipped mean it was sampled around (cem_planner_set_mean_candidate;
        mean_candidate restates the kernel).  Sticky."""
        _capi.check(self.lib.cem_planner_set_mean_candidate(self.h, 1 if enable else 0), 'cem_planner_set_mean_candidate')

    def mean_candidate(self):
        on = C.c_int32()
        _capi.check(self.lib.cem_planner_get_mean_candidate(self.h, C.byref(on)), 'cem_planner_get_mean_candidate')
        return bool(on.value)

    def set_plan_readout(self, on=True):
        """The plan read-out (cem_planner_set_plan_readout): a tracker kernel behind every select keeps the best-so-far candidate's whole
        action sequence, its per-particle returns and per-step cost counts (plan_readout reads them; track_best restates the kernel).
        Sticky; waits for the stream and re-captures the graph.  Sampler, rollout, select and refit launch as before."""
        _capi.check(self.lib.cem_planner_set_plan_readout(self.h, 1 if on else 0), 'cem_planner_set_plan_readout')

    def plan_readout_enabled(self):
        on = C.c_int32()
        _capi.check(self.lib.cem_planner_get_plan_readout(self.h, C.byref(on)), 'cem_planner_get_plan_readout')
        return bool(on.value)

    def plan_readout(self, problem=0) -> 'PlanReadout':
        """The read-out block of `problem` (cem_planner_plan_readout) as a PlanReadout.  Waits for the planner's stream: plan() returns
        as soon as action, score and iterations are on the host, and the last iteration's tracker runs behind that."""
        c = self.cfg
        seq = np.zeros((c.horizon, c.act_dim), np.float32)
        pret = np.zeros(c.particles, np.float32)
        cnt = np.zeros(c.horizon, np.int32)
        head = _capi.CemPlanReadout()
        _capi.check(self.lib.cem_planner_plan_readout(self.h, int(problem), C.byref(head), _np_ptr(seq), _np_ptr(pret), _np_ptr(cnt)),
                    'cem_planner_plan_readout')
        return PlanReadout(seq, np.float32(head.score), int(head.candidate), int(head.iteration), pret, cnt, int(head.flags))

    def set_task(self, task=None):
        """Score rollouts by a QuadraticTask instead of the Safety-Gym scorer (cem_planner_set_task); None switches it off.  While on,
        every iteration launches the sampler, the MODE 1 rollout kernel and cem_task_score_kernel; rollout_path() is 'generic'.
        Sticky; waits for the stream and re-captures the graph.  task_objective restates the kernel.  A task with `zones` has them
        applied in the same call (cem_planner_set_task_zones: cem_task_zones_kernel then scores); a task without clears any."""
        if task is None:
            _capi.check(self.lib.cem_planner_set_task(self.h, None), 'cem_planner_set_task')
            self.task, self.task_clock = None, None
            return
        tb = task.tables(self.cfg.obs_dim, self.cfg.act_dim)      # (kept alive until the call returns: the library copies them)
        zt = task.zone_tables(self.cfg.obs_dim)                   # (refused before anything of the handle changes)
        ot = task.output_tables(self.cfg.obs_dim)
        self._set_task_base(task, tb)
        if zt is not None or ot is not None:
            # outputs (cem_planner_set_task_outputs), then zones (cem_planner_set_task_zones): cem_task_outputs_kernel /
            # cem_task_zones_kernel in the task kernel's place; the objectives restate them
            try:
                if ot is not None:
                    self._set_task_outputs(ot)
                if zt is not None:
                    self._set_task_zones(zt)
            except Exception:
                _capi.check(self.lib.cem_planner_set_task(self.h, None), 'cem_planner_set_task')     # (not half a task: none)
                self.task, self.task_clock = None, None
                raise

    @property
    def task_zones(self):
        """The StateZones of the task in force, or None."""
        return getattr(self.task, 'zones', None)

    def set_task_zones(self, zones=None):
        """The StateZones of the task in force (cem_planner_set_task_zones); None clears them.  Sticky until the next set_task; waits
        for the stream and re-captures the graph."""
        if zones is None:
            _capi.check(self.lib.cem_planner_set_task_zones(self.h, None), 'cem_planner_set_task_zones')
        else:
            if not isinstance(zones, StateZones):
                raise ValueError('zones must be a StateZones')
            ot = self.task.output_tables(self.cfg.obs_dim) if self.task is not None else None
            self._set_task_zones(zones.tables(self.cfg.obs_dim + (ot['matrix'].shape[0] if ot is not None else 0)))
        if self.task is not None:
            self.task = _dc_replace(self.task, zones=zones)

    @property
    def task_outputs(self):
        """The TaskOutputs of the task in force, or None."""
        return getattr(self.task, 'outputs', None)

    def set_task_outputs(self, outputs=None):
        """The TaskOutputs of the task in force (cem_planner_set_task_outputs); None clears them.  Either way the zones are cleared:
        set the outputs, then the zones (which may then name outputs as axes).  Sticky until the next set_task; waits for the stream
        and re-captures the graph."""
        if outputs is None:
            had = self.task_outputs is not None
            _capi.check(self.lib.cem_planner_set_task_outputs(self.h, None), 'cem_planner_set_task_outputs')
            if self.task is not None and had:
                self.task = _dc_replace(self.task, outputs=None, zones=None)
            return
        if not isinstance(outputs, TaskOutputs):
            raise ValueError('outputs must be a TaskOutputs')
        ref = getattr(self.task, 'reference', None)
        self._set_task_outputs(outputs.tables(self.cfg.obs_dim, ref_rows=np.asarray(ref).shape[0] if ref is not None else 1))
        if self.task is not None:
            self.task = _dc_replace(self.task, outputs=outputs, zones=None)

    def _set_task_outputs(self, ot):
        fp = C.POINTER(C.c_float)
        per_step = ot['target'].shape[0] > 1
        co = _capi.CemTaskOutputs(n_outputs=ot['matrix'].shape[0], matrix=ot['matrix'].ctypes.data_as(fp), weight=ot['weight'].ctypes.data_as(fp),
                                  target=ot['target'].ctypes.data_as(fp), linear=ot['linear'].ctypes.data_as(fp), near=ot['near'].ctypes.data_as(fp),
                                  lo=ot['lo'].ctypes.data_as(fp), hi=ot['hi'].ctypes.data_as(fp),
                                  terminal=ot['terminal'].ctypes.data_as(fp) if ot['terminal'] is not None else None,
                                  ref_rows=ot['target'].shape[0] if per_step else 0,
                                  reference=ot['target'].ctypes.data_as(fp) if per_step else None)
        _capi.check(self.lib.cem_planner_set_task_outputs(self.h, C.byref(co)), 'cem_planner_set_task_outputs')

    def _set_task_zones(self, zt):
        fp, ip = C.POINTER(C.c_float), C.POINTER(C.c_int32)
        cz = _capi.CemTaskZones(n_zones=zt['axis'].shape[0], axis=zt['axis'].ctypes.data_as(ip), centre=zt['centre'].ctypes.data_as(fp),
                                weight=zt['weight'].ctypes.data_as(fp), radius=zt['radius'].ctypes.data_as(fp),
                                margin=zt['margin'].ctypes.data_as(fp), penalty=zt['penalty'].ctypes.data_as(fp),
                                keep_in=zt['keep_in'].ctypes.data_as(ip))
        _capi.check(self.lib.cem_planner_set_task_zones(self.h, C.byref(cz)), 'cem_planner_set_task_zones')

    def _set_task_base(self, task, tb):
        fp = C.POINTER(C.c_float)
        if isinstance(task, TrackingTask):
            # a TrackingTask (cem_planner_set_task_tracking): the same launches with cem_task_reference_kernel behind the rollout;
            # the clock starts at (0, zeros); tracking_objective restates the kernel
            base = _capi.CemTask(kind=_capi.CEM_TASK_QUADRATIC, goal_radius=float(task.goal_radius), reward_goal=float(task.reward_goal),
                                 reward_clip=float(task.reward_clip),
                                 **{k: tb[k].ctypes.data_as(fp) for k in ('q', 'c', 'goal_mask', 'lo', 'hi', 'rho')})
            trk = _capi.CemTaskTracking(ref=tb['reference'].ctypes.data_as(fp), ref_steps=tb['reference'].shape[0],
                                        q_terminal=tb['q_terminal'].ctypes.data_as(fp) if task.terminal_weights is not None else None,
                                        action_rate=tb['action_rate'].ctypes.data_as(fp) if task.action_rate is not None else None)
            _capi.check(self.lib.cem_planner_set_task_tracking(self.h, C.byref(base), C.byref(trk)), 'cem_planner_set_task_tracking')
            self.task, self.task_clock = task, (0, np.zeros(self.cfg.act_dim, np.float32))
            return
        ct = _capi.CemTask(kind=_capi.CEM_TASK_QUADRATIC, goal_radius=float(task.goal_radius), reward_goal=float(task.reward_goal),
                           reward_clip=float(task.reward_clip), **{k: tb[k].ctypes.data_as(fp) for k in tb})
        _capi.check(self.lib.cem_planner_set_task(self.h, C.byref(ct)), 'cem_planner_set_task')
        self.task, self.task_clock = task, None

    def set_task_clock(self, k0, prev_action=None):
        """The clock of a TrackingTask (cem_planner_set_task_clock): the plan's first state is compared with reference row k0, its first
        action with prev_action [act_dim] (None: as it was).  A stream-ordered copy: later plans see it, the captured graph stays.
        `task_clock` is the host's record of it."""
        a = None if prev_action is None else np.ascontiguousarray(np.asarray(prev_action, np.float32).reshape(self.cfg.act_dim))
        _capi.check(self.lib.cem_planner_set_task_clock(self.h, int(k0), _np_ptr(a) if a is not None else None), 'cem_planner_set_task_clock')
        self.task_clock = (int(k0), a.copy() if a is not None else self.task_clock[1])

    def task_trajectories(self):
        """The raw state trajectories [P * n_samples, H + 1, obs_dim] of the last rollout launch of a task plan, a copy (torch, on the
        GPU; cem_planner_task_trajectories).  Rows p * n + candidate; an iteration of a population schedule fills the leading P * n[it]."""
        c, t = self.cfg, self._torch
        out = t.empty((c.particles * self.n_local, c.horizon + 1, c.obs_dim), dtype=t.float32, device=self.device)
        self._wait_inputs()
        _capi.check(self.lib.cem_planner_task_trajectories(self.h, _ptr(out)), 'cem_planner_task_trajectories')
        return out

    def task_score(self, trajectories, actions):
        """cem_task_score_kernel alone (cem_task_score) with the handle's task and variant: trajectories [P * n, H + 1, obs_dim], actions
        [n, H, act_dim] -> (returns [P * n] float32, cost bytes [H, P * n] uint8 — None on a 'cem' handle), torch tensors on the GPU."""
        c, t = self.cfg, self._torch
        traj = t.as_tensor(trajectories, dtype=t.float32, device=self.device).contiguous()
        act = t.as_tensor(actions, dtype=t.float32, device=self.device).contiguous()
        if traj.dim() != 3 or traj.shape[2] != c.obs_dim or traj.shape[1] < 2:
            raise ValueError('trajectories must be [P*n, H+1, obs_dim]')
        B, H = traj.shape[0], traj.shape[1] - 1
        if B % c.particles != 0 or tuple(act.shape) != (B // c.particles, H, c.act_dim):
            raise ValueError('actions must be [rows / particles, H, act_dim]')
        ret = t.empty((B,), dtype=t.float32, device=self.device)
        costs = t.empty((H, B), dtype=t.uint8, device=self.device) if c.variant != 'cem' else None
        self._wait_inputs()
        _capi.check(self.lib.cem_task_score(self.h, _ptr(traj), _ptr(act), B, H, _ptr(ret), _ptr(costs)), 'cem_task_score')
        return ret, costs

    def plan_exchange(self):
        _capi.check(self.lib.cem_plan_exchange(self.h), 'cem_plan_exchange')

    def select_mode(self):
        """The select form the next iteration takes on this handle: 1 one workgroup, 2 the multi-launch chain, 3 the chain fused into one
        launch (cem_planner_select_mode; 2 for good once a fused select had to be recovered)."""
        m = C.c_int32()
        _capi.check(self.lib.cem_planner_select_mode(self.h, C.byref(m)), 'cem_planner_select_mode')
        return m.value

    def select_form(self, it=0):
        """0 cem_select_kernel (and every select that is not one workgroup) | 1 cem_select_ranked_kernel: which form of the one-workgroup
        select iteration `it` launches (cem_planner_select_form).  Same results; CEM_FORCE_SELECT=bucket at create keeps form 0."""
        n = C.c_int32()
        _capi.check(self.lib.cem_planner_select_form(self.h, int(it), C.byref(n)), 'cem_planner_select_form')
        return n.value

    def inject_fault(self, kind=1):
        """Test hook (cem_planner_inject_fault): the next plan's first fused select sees one of its grid barriers expire."""
        _capi.check(self.lib.cem_planner_inject_fault(self.h, kind), 'cem_planner_inject_fault')

    # ------------------------------------------------------------------ warm start (cem_mpc.h: cem_init_mode)
    # The handle keeps, per slot, the mu / sigma its last completed plan ended with (the carry).  A slot's next plan starts from the
    # action box ('cold': the reference's behaviour and the default), from arrays the caller uploaded ('explicit') or from the carry
    # shifted towards the present ('shift'; cold while the carry is invalid).  A single-state handle has one slot, 0.
    # The carry lives on the HANDLE: two users of one handle (cached_planner) would continue each other's plans, so anything that
    # warm-starts must own its handle (owner= of cached_planner / cached_batch_planner).
    INIT_MODES = {'cold': _capi.CEM_INIT_COLD, 'explicit': _capi.CEM_INIT_EXPLICIT, 'shift': _capi.CEM_INIT_SHIFT}

    def n_slots(self):
        return self.max_batch

    def set_warm_start(self, shift=1, tail='box', sigma='reset', floor_frac=0.0):
        """Parameters of the 'shift' mode: mu moves `shift` steps; the freed tail takes the box centre ('box') or repeats the last step
        ('repeat'); sigma restarts from the box ('reset', PETS) or is kept, floored at fl32(floor_frac * sigma0) per dimension ('keep')."""
        tails, rules = {'box': 0, 'repeat': 1}, {'reset': 0, 'keep': 1}
        if tail not in tails or sigma not in rules:
            raise ValueError("tail is 'box' or 'repeat', sigma is 'reset' or 'keep'")
        ws = _capi.CemWarmStart(shift=int(shift), tail=tails[tail], sigma_rule=rules[sigma])
        ws.sigma_floor[:self.cfg.act_dim] = warm_sigma_floor(self.cfg, floor_frac).tolist()
        _capi.check(self.lib.cem_planner_set_warm_start(self.h, C.byref(ws)), 'cem_planner_set_warm_start')

    def set_initial_distribution(self, mu, sigma, slot=0):
        """mu[H, A], sigma[H, A] of the 'explicit' mode for `slot` (the mode itself is set by set_init_mode)."""
        c = self.cfg
        m = np.ascontiguousarray(np.asarray(mu, np.float32))
        s = np.ascontiguousarray(np.asarray(sigma, np.float32))
        if m.shape != (c.horizon, c.act_dim) or s.shape != (c.horizon, c.act_dim):
            raise ValueError('mu and sigma must have shape [%d, %d]' % (c.horizon, c.act_dim))
        _capi.check(self.lib.cem_planner_set_initial_distribution(self.h, int(slot), _np_ptr(m), _np_ptr(s)), 'cem_planner_set_initial_distribution')

    def set_init_mode(self, mode, slot=0):
        """'cold' | 'explicit' | 'shift' (or the enum value) for `slot` (None: every slot); sticky until changed."""
        m = self.INIT_MODES[mode] if isinstance(mode, str) else int(mode)
        _capi.check(self.lib.cem_planner_set_init_mode(self.h, -1 if slot is None else int(slot), m), 'cem_planner_set_init_mode')

    def reset_carry(self, slot=None):
        """Forget the carry of `slot` (None: of every slot): its next 'shift' plan starts cold."""
        _capi.check(self.lib.cem_planner_reset_carry(self.h, -1 if slot is None else int(slot)), 'cem_planner_reset_carry')

    def carry(self, slot=0):
        """(mu[H, A], sigma[H, A], valid) of the slot's last completed plan; zeros while invalid.  Waits for the planner's stream."""
        c = self.cfg
        m, s = np.zeros((c.horizon, c.act_dim), np.float32), np.zeros((c.horizon, c.act_dim), np.float32)
        v = C.c_int32()
        _capi.check(self.lib.cem_planner_get_carry(self.h, int(slot), _np_ptr(m), _np_ptr(s), C.byref(v)), 'cem_planner_get_carry')
        return m, s, bool(v.value)

    # ------------------------------------------------------------------ planning
    def _noise_args(self, eps_act, eps_model, lead=()):
        """The explicit noise tensors on the device, shapes checked; lead = (B,) for the rows of a batched plan."""
        c = self.cfg
        t = self._torch
        if eps_act is None and eps_model is None:
            return None, None
        if eps_act is None or eps_model is None:
            raise ValueError('eps_act and eps_model must be given together')
        ea = t.as_tensor(eps_act, dtype=t.float32, device=self.device).contiguous()
        em = t.as_tensor(eps_model, dtype=t.float32, device=self.device).contiguous()
        b = 'B,' if lead else ''
        if tuple(ea.shape) != tuple(lead) + (c.iterations, c.n_samples, c.horizon, c.act_dim):
            raise ValueError('eps_act must be [%sI,N,H,A]' % b)
        if tuple(em.shape) != tuple(lead) + (c.iterations, c.horizon, c.particles * c.n_samples, c.obs_dim):
            raise ValueError('eps_model must be [%sI,H,P*N,O]' % b)
        return ea, em

    def take_calls(self, n=1):
        """The next n call numbers of the handle's counter (what plan / plan_batch draw when given none), as uint64 [n]; the counter advances."""
        first = self._call
        self._call += int(n)
        return np.arange(first, first + int(n), dtype=np.uint64)

    def plan(self, state, seed=0, call=None, eps_act=None, eps_model=None, eps_out=None):
        """CemMpc.generate_action (cem_mpc.py:31-33): state[O] -> (action[A], best_score, iters)."""
        if np.shape(state) != self._st_buf.shape:
            raise ValueError('state must have shape [%d]' % self.cfg.obs_dim)
        self._st_buf[:] = state                                     # (float64 observations are cast here, as cem_mpc.py:32 does)
        if call is None:
            call = self._call
            self._call += 1
        if eps_act is None and eps_model is None and eps_out is None:     # the generator path: nothing else to marshal
            st = self.lib.cem_planner_plan(self.h, self._st_ptr, seed, call, None, None, None, self._act_ptr, self._score_ref, self._iters_ref)
            if st:
                _capi.check(st, 'cem_planner_plan')
            return self._act_buf.copy(), self._score.value, self._iters.value
        ea, em = self._noise_args(eps_act, eps_model)
        eo = np.ascontiguousarray(np.asarray(eps_out, np.float32)) if eps_out is not None else None
        if ea is not None:
            self._wait_inputs()
        _capi.check(self.lib.cem_planner_plan(self.h, self._st_ptr, seed, call, _ptr(ea), _ptr(em), _np_ptr(eo),
                                              self._act_ptr, self._score_ref, self._iters_ref), 'cem_planner_plan')
        return self._act_buf.copy(), float(self._score.value), int(self._iters.value)

    def plan_begin(self, state, seed=0, call=0, eps_act=None, eps_model=None):
        st = np.ascontiguousarray(np.asarray(state, np.float32))
        ea, em = self._noise_args(eps_act, eps_model)
        self._keep = (ea, em)
        self._wait_inputs()
        _capi.check(self.lib.cem_plan_begin(self.h, _np_ptr(st), seed, call, _ptr(ea), _ptr(em)), 'cem_plan_begin')

    def plan_rollout(self, it):
        _capi.check(self.lib.cem_plan_rollout(self.h, it), 'cem_plan_rollout')

    def plan_select(self, it):
        _capi.check(self.lib.cem_plan_select(self.h, it), 'cem_plan_select')

    def plan_end(self, eps_out=None):
        c = self.cfg
        eo = np.ascontiguousarray(np.asarray(eps_out, np.float32)) if eps_out is not None else None
        action = np.zeros(c.act_dim, np.float32)
        score = C.c_float()
        iters = C.c_int32()
        _capi.check(self.lib.cem_plan_end(self.h, _np_ptr(eo), _np_ptr(action), C.byref(score), C.byref(iters)), 'cem_plan_end')
        self._keep = None
        return action, float(score.value), int(iters.value)

    # ------------------------------------------------------------------ model API
    def unfold_sequences(self, s0, actions, eps_model=None, seed=0, call=0, return_moments=False):
        """TransitionModel.unfold_sequences (transition_model.py:64-77) on device:
        s0 [B,O], actions [B,H,A] -> traj [B,H+1,O] (torch tensors on the GPU)."""
        t = self._torch
        c = self.cfg
        s0 = t.as_tensor(s0, dtype=t.float32, device=self.device).contiguous()
        actions = t.as_tensor(actions, dtype=t.float32, device=self.device).contiguous()
        B, H = actions.shape[0], actions.shape[1]
        if tuple(s0.shape) != (B, c.obs_dim) or actions.shape[2] != c.act_dim:
            raise ValueError('bad shapes for unfold_sequences')
        em = None
        if eps_model is not None:
            em = t.as_tensor(eps_model, dtype=t.float32, device=self.device).contiguous()
            if tuple(em.shape) != (H, B, c.obs_dim):
                raise ValueError('eps_model must be [H,B,O]')
        traj = t.empty((B, H + 1, c.obs_dim), dtype=t.float32, device=self.device)
        mu = t.empty((B, H, c.obs_dim), dtype=t.float32, device=self.device) if return_moments else None
        sd = t.empty((B, H, c.obs_dim), dtype=t.float32, device=self.device) if return_moments else None
        self._wait_inputs()
        _capi.check(self.lib.cem_unfold_sequences(self.h, _ptr(s0), _ptr(actions), B, H, _ptr(em), seed, call,
                                                  _ptr(traj), _ptr(mu), _ptr(sd)), 'cem_unfold_sequences')
        return (traj, mu, sd) if return_moments else traj

    def compute_objective(self, trajectories):
        """MpcPolicy.compute_objective (mpc_policy.py:26-39) / SafeCemMpc.compute_objective (safe_cem_mpc.py:76-96) on a
        given trajectory tensor [P*n, H+1, O] (rows in the tf.tile order p*n + candidate) -> scores [n] (torch, on the GPU).
        A 'cost' handle returns the planner's objective -compute_mean_costs (safe_cem_mpc.py:98-108): minus the mean cost, <= 0."""
        t = self._torch
        c = self.cfg
        traj = t.as_tensor(trajectories, dtype=t.float32, device=self.device).contiguous()
        if traj.dim() != 3 or traj.shape[2] != c.obs_dim or traj.shape[1] < 2:
            raise ValueError('trajectories must be [P*n, H+1, obs_dim]')
        B, H = traj.shape[0], traj.shape[1] - 1
        if B % c.particles != 0:
            raise ValueError('trajectory rows (%d) are not a multiple of particles (%d)' % (B, c.particles))
        scores = t.empty((B // c.particles,), dtype=t.float32, device=self.device)
        self._wait_inputs()
        _capi.check(self.lib.cem_compute_objective(self.h, _ptr(traj), B, H, _ptr(scores)), 'cem_compute_objective')
        return scores

    def scorer_reward(self, observations, next_observations):
        """SafetyGymStateScorer.reward (safety_gym.py:110-119,140-143): (reward [n] float32, goal_achieved [n] bool)."""
        t = self._torch
        obs = t.as_tensor(observations, dtype=t.float32, device=self.device).contiguous()
        nxt = t.as_tensor(next_observations, dtype=t.float32, device=self.device).contiguous()
        if obs.dim() != 2 or obs.shape[1] != self.cfg.obs_dim or nxt.shape != obs.shape:
            raise ValueError('observations / next_observations must both be [n, obs_dim]')
        r = t.empty((obs.shape[0],), dtype=t.float32, device=self.device)
        g = t.empty((obs.shape[0],), dtype=t.uint8, device=self.device)
        self._wait_inputs()
        _capi.check(self.lib.cem_scorer_reward(self.h, _ptr(obs), _ptr(nxt), obs.shape[0], _ptr(r), _ptr(g)), 'cem_scorer_reward')
        return r, g.bool()

    def scorer_cost(self, observations):
        """SafetyGymStateScorer.cost (safety_gym.py:145-166): cost [n] float32."""
        t = self._torch
        obs = t.as_tensor(observations, dtype=t.float32, device=self.device).contiguous()
        if obs.dim() != 2 or obs.shape[1] != self.cfg.obs_dim:
            raise ValueError('observations must be [n, obs_dim]')
        c = t.empty((obs.shape[0],), dtype=t.float32, device=self.device)
        self._wait_inputs()
        _capi.check(self.lib.cem_scorer_cost(self.h, _ptr(obs), obs.shape[0], _ptr(c)), 'cem_scorer_cost')
        return c

    def fill_noise(self, seed=0, call=0):
        """The Philox streams a (seed, call) plan consumes, as explicit tensors."""
        t = self._torch
        c = self.cfg
        B = c.particles * c.n_samples
        ea = t.empty((c.iterations, c.n_samples, c.horizon, c.act_dim), dtype=t.float32, device=self.device)
        em = t.empty((c.iterations, c.horizon, B, c.obs_dim), dtype=t.float32, device=self.device)
        eo = t.empty((c.act_dim,), dtype=t.float32, device=self.device)
        self._wait_inputs()
        _capi.check(self.lib.cem_fill_noise(self.h, seed, call, _ptr(ea), _ptr(em), _ptr(eo)), 'cem_fill_noise')
        return ea, em, eo

    def output_noise(self, seed=0, call=0) -> np.ndarray:
        """eps_out [A] of a (seed, call) plan alone (cem_fill_noise with no other tensor): the standard normals a plan's result adds,
        scaled by noise_stddev, to the first action of its best sequence."""
        eo = self._torch.empty((self.cfg.act_dim,), dtype=self._torch.float32, device=self.device)
        self._wait_inputs()
        _capi.check(self.lib.cem_fill_noise(self.h, seed, call, None, None, _ptr(eo)), 'cem_fill_noise')
        return eo.cpu().numpy()

    def philox_words(self, seed, call, stream, iteration, t, sub, idx0, n):
        """The generator's raw Philox4x32-7 output words for n consecutive counters (test hook, cem_mpc.h): uint32 [n, 4]."""
        out = self._torch.empty((n, 4), dtype=self._torch.int32, device=self.device)
        self._wait_inputs()
        _capi.check(self.lib.cem_philox_words(self.h, seed, call, stream, iteration, t, sub, idx0, n, _ptr(out)), 'cem_philox_words')
        return out.cpu().numpy().view('uint32')

    def set_timing(self, enable=True):
        _capi.check(self.lib.cem_planner_set_timing(self.h, int(enable)), 'cem_planner_set_timing')

    def last_timing(self):
        r, n, s = C.c_float(), C.c_int32(), C.c_float()
        _capi.check(self.lib.cem_planner_last_timing(self.h, C.byref(r), C.byref(n), C.byref(s)), 'cem_planner_last_timing')
        rd, sa = C.c_float(), C.c_float()
        _capi.check(self.lib.cem_planner_last_timing_detail(self.h, C.byref(rd), C.byref(sa)), 'cem_planner_last_timing_detail')
        return dict(rollout_ms=float(r.value), rollout_launches=int(n.value), select_ms=float(s.value), reduce_ms=float(rd.value),
                    sampler_ms=float(sa.value))

    def tiles(self):
        """(chunks_per_tile, tiles[n,6]) of this handle's plan (host-side logic, no GPU call)."""
        return plan_tiles(self.cfg)

    def segments(self):
        return plan_segments(self.cfg)

    def close(self):
        if getattr(self, 'h', None):
            self.lib.cem_planner_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BatchCemPlanner(CemPlanner):
    """One batch handle (cem_batch_planner_create): up to ``max_batch`` observations per plan call, all problems side by side in one
    launch per stage.  Problem b of ``plan_batch`` returns bit for bit what ``CemPlanner.plan(states[b], seed, calls[b])`` returns on a
    single-state handle of the same configuration.  Weights, normaliser, timing and the workspace views are CemPlanner's (the per-problem
    arrays of the layout are [max_batch] consecutive slices); the single-state and stepwise calls raise (CEM_ERR_STATE)."""

    def __init__(self, cfg: PlannerConfig, max_batch: int, device='cuda:0'):
        self.max_batch = int(max_batch)
        super().__init__(cfg, device=device)          # (CemPlanner.plan's staging too: the library refuses a single-state call, CEM_ERR_STATE)
        # staging for the hot path, made once (as CemPlanner.plan's)
        mb, O, A = self.max_batch, cfg.obs_dim, cfg.act_dim
        self._states_buf = np.zeros((mb, O), np.float32)
        self._calls_buf = np.zeros(mb, np.uint64)
        self._acts_buf = np.zeros((mb, A), np.float32)
        self._scores_buf = np.zeros(mb, np.float32)
        self._iters_buf = np.zeros(mb, np.int32)
        self._b_ptrs = tuple(_np_ptr(a) for a in (self._states_buf, self._calls_buf, self._acts_buf, self._scores_buf, self._iters_buf))

    def _workspace_bytes(self):
        return self.lib.cem_batch_workspace_bytes(C.byref(self.ccfg), self.max_batch)

    def _create(self, ws_ptr, nbytes, stream, out):
        _capi.check(self.lib.cem_batch_planner_create(C.byref(self.ccfg), self.max_batch, ws_ptr, nbytes, stream, out), 'cem_batch_planner_create')

    def batch_capacity(self):
        n = C.c_int32()
        _capi.check(self.lib.cem_planner_batch_capacity(self.h, C.byref(n)), 'cem_planner_batch_capacity')
        return n.value

    def set_carry_slots(self, slots=None):
        """Problem b of the following plan_batch calls reads and writes carry slot slots[b] (distinct, in [0, max_batch)); None: b."""
        if slots is None:
            _capi.check(self.lib.cem_planner_set_carry_slots(self.h, self.max_batch, None), 'cem_planner_set_carry_slots')
            return
        sl = np.ascontiguousarray(np.asarray(slots, np.int32).reshape(-1))
        _capi.check(self.lib.cem_planner_set_carry_slots(self.h, sl.size, _np_ptr(sl)), 'cem_planner_set_carry_slots')

    def plan_batch(self, states, seed=0, calls=None, eps_act=None, eps_model=None, eps_out=None, slots=None):
        """CemMpc.generate_action for every row of states[B, O] in ONE plan call -> (actions[B, A], scores[B], iters[B]).
        calls=None draws B consecutive call numbers from the handle's counter.  slots[B] (warm start): the carry slot of every row,
        e.g. its environment's index when the rows are a compacted subset; the map stays for later calls; None leaves it as it is
        (initially row b -> slot b)."""
        if slots is not None:
            if np.size(slots) != np.shape(states)[0]:
                raise ValueError('slots must have one entry per row of states')
            self.set_carry_slots(slots)
        st = np.asarray(states)
        if st.ndim != 2 or st.shape[1] != self.cfg.obs_dim:
            raise ValueError('states must have shape [B, %d]' % self.cfg.obs_dim)
        n = st.shape[0]
        sp, cp, ap, scp, ip = self._b_ptrs
        if n < 1 or n > self.max_batch:                 # the library's own check (CEM_ERR_INVALID_ARG); nothing is staged
            _capi.check(self.lib.cem_planner_plan_batch(self.h, n, sp, seed, cp, None, None, None, ap, scp, ip), 'cem_planner_plan_batch')
        self._states_buf[:n] = st
        if calls is None:
            self._calls_buf[:n] = np.arange(self._call, self._call + n, dtype=np.uint64)
            self._call += n
        else:
            cl = np.asarray(calls, np.uint64).reshape(-1)
            if cl.shape != (n,):
                raise ValueError('calls must have shape [B]')
            self._calls_buf[:n] = cl
        if eps_act is None and eps_model is None and eps_out is None:
            st_ = self.lib.cem_planner_plan_batch(self.h, n, sp, seed, cp, None, None, None, ap, scp, ip)
            if st_:
                _capi.check(st_, 'cem_planner_plan_batch')
        else:
            ea, em = self._noise_args(eps_act, eps_model, lead=(n,))
            eo = None
            if eps_out is not None:
                eo = np.ascontiguousarray(np.asarray(eps_out, np.float32))
                if eo.shape != (n, self.cfg.act_dim):
                    raise ValueError('eps_out must be [B,A]')
            if ea is not None:
                self._wait_inputs()
            _capi.check(self.lib.cem_planner_plan_batch(self.h, n, sp, seed, cp, _ptr(ea), _ptr(em), _np_ptr(eo), ap, scp, ip),
                        'cem_planner_plan_batch')
        return self._acts_buf[:n].copy(), self._scores_buf[:n].copy(), self._iters_buf[:n].copy()


def stage_model_weights(planner, ensemble):
    """The weight sync of the model-holding classes (TransitionModel._get_planner, the policies): on the device when the ensemble's
    weights live there (MlpEnsemble.weights_device) on the planner's device and the planner can take them (a stand-in that only knows
    set_weights cannot), else over the host as before.  The trainer's stream is drained wherever it last wrote the weights (fit,
    set_state), so the planner's stream needs no more than its usual wait on the current stream."""
    get_dev = getattr(ensemble, 'weights_device', None)
    blob = get_dev() if get_dev is not None and hasattr(planner, 'set_weights_dev') else None
    if blob is not None and blob.device == planner.device:
        planner.set_weights_dev(blob)
        ensemble.weights_read_on(planner.stream)         # the trainer's next write of the blob waits for the pack kernels
    else:
        planner.set_weights(ensemble.get_weights())


def warm_sigma_floor(cfg: PlannerConfig, floor_frac) -> np.ndarray:
    """sigma_floor[A] of cem_warm_start_t: fl32(fl32(floor_frac) * sigma0), sigma0 as the handle's configuration carries it."""
    sigma0 = sampling_params(cfg.act_low, cfg.act_high)[3]
    return (np.float32(floor_frac) * np.asarray(sigma0, np.float32)).astype(np.float32)


def shift_distribution(mu, sigma, mu0, sigma0, shift=1, tail=0, sigma_rule=0, sigma_floor=None):
    """Host restatement of CEM_INIT_SHIFT (cem_mpc.h) — copies and one max, so it is exact: (mu_init, sigma_init) [H, A] from a carry."""
    mu, sigma = np.asarray(mu, np.float32), np.asarray(sigma, np.float32)
    H = mu.shape[0]
    if not 1 <= shift < H:
        raise ValueError('shift must lie in 1 .. H - 1')
    m = np.broadcast_to(np.asarray(mu0, np.float32), mu.shape).copy()
    s = np.broadcast_to(np.asarray(sigma0, np.float32), mu.shape).copy()
    m[:H - shift] = mu[shift:]
    if tail:
        m[H - shift:] = mu[H - 1]
    if sigma_rule:
        s[:H - shift] = np.maximum(sigma[shift:], np.asarray(sigma_floor, np.float32))
    return m, s


def softmax_refit(scores, elite, actions, mu, sigma, smoothing, temperature):
    """Host restatement of one CEM_REFIT_SOFTMAX iteration (cem_mpc.h) for users, in fp32 with NumPy's own summation order — the device's
    values, not its bits.  scores [N], elite [k] candidate indices, actions [N, H, A] (or [N, H * A]), mu / sigma of the actions' trailing
    shape -> (mu_new, sigma_new, ess)."""
    f = np.float32
    tau = f(temperature)
    if not (np.isfinite(tau) and tau > 0):
        raise ValueError('temperature must be finite and > 0')
    e = np.asarray(elite, np.int64).reshape(-1)
    s = np.asarray(scores, f)[e]
    a = np.asarray(actions, f)[e]
    mu, sigma = np.asarray(mu, f), np.asarray(sigma, f)
    if a.shape[1:] != mu.shape or sigma.shape != mu.shape:
        raise ValueError('mu / sigma must have the shape of one action row')
    smax = s.max()
    beta = f(1.0) / tau
    with np.errstate(invalid='ignore', over='ignore', under='ignore'):
        w = np.where(s == smax, f(1.0), np.exp(((s - smax) * beta).astype(f)).astype(f)).astype(f)
    W = w.sum(dtype=f)
    wb = w.reshape((-1,) + (1,) * mu.ndim)
    mean = ((wb * a).sum(axis=0, dtype=f) / W).astype(f)
    d = (a - mean).astype(f)
    var = ((wb * (d * d)).sum(axis=0, dtype=f) / W).astype(f)
    sm, osm = f(smoothing), f(1.0 - float(smoothing))
    return (sm * mu + osm * mean).astype(f), (sm * sigma + osm * np.sqrt(var)).astype(f), f(W * W / (w * w).sum(dtype=f))


def score_keys(scores) -> np.ndarray:
    """The uint32 keys the selects rank fp32 scores by (cem_f2key): a larger key is a better score, -0.0 and +0.0 share a key, every
    NaN has key 0 (below -inf)."""
    u = np.ascontiguousarray(np.asarray(scores, np.float32)).view(np.uint32)
    nan = (u & np.uint32(0x7fffffff)) > np.uint32(0x7f800000)
    neg = ((u & np.uint32(0x80000000)) != 0) & (u != np.uint32(0x80000000))
    return np.where(nan, np.uint32(0), np.where(neg, ~u, u | np.uint32(0x80000000))).astype(np.uint32)


def keep_elites(scores, elite_idx, actions, m) -> np.ndarray:
    """Host restatement of cem_elite_keep_kernel (cem_mpc.h, cem_planner_set_elite_carry) — comparisons and copies, so it is exact:
    E [m, H, A], the best m of the k elites.  scores [N] as the select ranked them, elite_idx [k] as it stored them, actions [N, H, A].
    Order: descending score key (score_keys), ties to the lower candidate index."""
    e = np.asarray(elite_idx, np.int64).reshape(-1)
    m = int(m)
    if not 0 <= m <= e.size:
        raise ValueError('m must lie in 0 .. k')
    key = score_keys(np.asarray(scores, np.float32).reshape(-1)[e]).astype(np.int64)
    order = np.lexsort((e, -key))                       # last key first: descending score key, then ascending candidate index
    return np.ascontiguousarray(np.asarray(actions, np.float32)[e[order[:m]]])


def inject_elites(actions, E, count, shift=0) -> np.ndarray:
    """Host restatement of cem_elite_inject_kernel — copies, so it is exact: a copy of actions [N, H, A] whose rows n < count hold
    E[n] moved `shift` steps towards the present at steps t < H - shift; later steps, later rows and everything at count == 0 keep what
    the sampler drew.  shift is the handle's at a plan's first iteration (across_plans), 0 at every other."""
    out = np.array(actions, np.float32, copy=True)
    E = np.asarray(E, np.float32)
    c, s, H = min(int(count), E.shape[0]), int(shift), out.shape[1]
    if not 0 <= s <= H:
        raise ValueError('shift must lie in 0 .. H')
    if c > 0:
        out[:c, :H - s] = E[:c, s:]
    return out


def elite_keep_count(fraction, n_elite) -> int:
    """Elites a policy keeps for a fraction in (0, 1] of n_elite (iCEM's 0.3): max(1, floor(fraction * n_elite))."""
    f = float(fraction)
    if not 0.0 < f <= 1.0:
        raise ValueError('keep_elites is a fraction of n_elite in (0, 1]')
    return max(1, int(np.floor(f * int(n_elite))))


def population_schedule(n_samples, n_elite, iterations, decay, particles, ensemble_size, min_population=None):
    """iCEM's population decay as a list of `iterations` sizes for cem_planner_set_population_schedule: iteration i gets
    ceil(n_samples / decay**i - 1e-9), not below min(n_samples, max(n_elite, min_population or 2 n_elite)), rounded up to a multiple of
    ensemble_size // gcd(particles, ensemble_size) (so that particles * n splits evenly among the members) and capped at n_samples.
    decay == 1 gives n_samples everywhere (off)."""
    import math
    N, k, I, P, E = int(n_samples), int(n_elite), int(iterations), int(particles), int(ensemble_size)
    g = float(decay)
    if not (math.isfinite(g) and g >= 1.0):
        raise ValueError('population decay must be finite and >= 1')
    if N < 1 or k < 1 or k > N or I < 1 or P < 1 or E < 1:
        raise ValueError('population_schedule needs 1 <= n_elite <= n_samples and positive iterations, particles, ensemble_size')
    if min_population is not None and int(min_population) < 1:
        raise ValueError('min_population must be positive')
    floor = min(N, max(k, int(min_population) if min_population is not None else 2 * k))
    q = E // math.gcd(P, E)
    out = []
    for i in range(I):
        n = max(int(math.ceil(N / g ** i - 1e-9)), floor)
        out.append(min(N, -(-n // q) * q))
    return out


def mean_candidate(actions, mu, lb, ub) -> np.ndarray:
    """Host restatement of cem_mean_candidate_kernel — a max, a min and copies, so it is exact: a copy of actions [n, H, A] whose LAST
    row is min(max(mu, lb), ub); mu [H, A] as the iteration samples from it, lb / ub [A]."""
    out = np.array(actions, np.float32, copy=True)
    m = np.asarray(mu, np.float32).reshape(out.shape[1:])
    out[-1] = np.minimum(np.maximum(m, np.asarray(lb, np.float32)), np.asarray(ub, np.float32))
    return out


def zone_terms(traj, zt):
    """The zones' part of cem_task_zones_kernel (csrc/cem_task_zones.h), bit for bit: traj [rows, H + 1, O] float32, zt the tables of
    StateZones.tables -> (hit [rows, H + 1] bool: the state hits a zone; pen [rows, H + 1] float32: the sixteen slots penalty * hinge
    added pairwise, neighbours first; slots [rows, H + 1, 16] float32).  Every product, difference and sum is a float32 operation of its own."""
    f = np.float32
    tr = np.asarray(traj, f)
    rows, H1, _ = tr.shape
    Z = zt['axis'].shape[0]
    slots = np.zeros((rows, H1, _capi.CEM_TASK_MAX_ZONES), f)
    hit = np.zeros((rows, H1), bool)
    with np.errstate(all='ignore'):
        for z in range(Z):
            dist2 = np.zeros((rows, H1), f)
            for d in range(_capi.CEM_TASK_ZONE_AXES):
                a = int(zt['axis'][z, d])
                if a < 0:
                    continue
                e = tr[:, :, a] - zt['centre'][z, d]
                dist2 = dist2 + zt['weight'][z, d] * (e * e)
            radius, margin = zt['radius'][z], zt['margin'][z]
            R2 = radius * radius
            if zt['keep_in'][z]:
                reach = radius - margin
                Rm2 = reach * reach
                hit |= dist2 > R2                                 # (a NaN compares false)
                gap = dist2 - Rm2
            else:
                reach = radius + margin
                Rm2 = reach * reach
                hit |= dist2 <= R2
                gap = Rm2 - dist2
            hinge = np.where(np.isnan(dist2) | ~(gap > 0), f(0), gap).astype(f)
            slots[:, :, z] = zt['penalty'][z] * hinge
        acc = slots
        for _ in range(4):
            acc = acc[..., 0::2] + acc[..., 1::2]
    return hit, acc[..., 0], slots


def output_terms(traj, ot):
    """The outputs y = C s of cem_task_outputs_kernel (csrc/cem_task_outputs.h), bit for bit: traj [rows, H + 1, O] float32, ot the tables
    of TaskOutputs.tables -> y [rows, H + 1, M] float32.  Sixteen partial sums per output, partial l over the features 64 i + 4 l + r (i,
    then r) from +0, every product and sum a float32 operation of its own; the sixteen added pairwise, neighbours first."""
    f = np.float32
    tr = np.asarray(traj, f)
    rows, H1, O = tr.shape
    Cm = np.zeros((ot['matrix'].shape[0], 128), f)
    Cm[:, :O] = ot['matrix']
    s = np.zeros((rows, H1, 128), f)
    s[..., :O] = tr
    s = s.reshape(rows, H1, 2, 16, 4)
    y = np.zeros((rows, H1, Cm.shape[0]), f)
    with np.errstate(all='ignore'):
        for m in range(Cm.shape[0]):
            cm = Cm[m].reshape(2, 16, 4)
            acc = np.zeros((rows, H1, 16), f)
            for i in range(2):
                for r in range(4):
                    acc = acc + cm[i, :, r] * s[:, :, i, :, r]
            for _ in range(4):
                acc = acc[..., 0::2] + acc[..., 1::2]
            y[..., m] = acc[..., 0]
    return y


def _task_objective(traj, actions, tb, ref, q_terminal, rate, task, variant, return_done, zt=None, ot=None, gy=None):
    """What task_objective and tracking_objective share, in the kernels' order: tb the [O] / [A] tables, ref [H + 1, O] the row every
    state is compared with (or [O]: one for all), q_terminal [O] the weights of the last state (None: q), rate [N, H] the action-rate
    term of every step (None: the reward has no such term), zt the zone tables (None: no zones, and the code of a task without), ot the
    output tables with gy [H + 1, M] the row every state's outputs are compared with (None: no outputs, and the code of a task without)."""
    f = np.float32
    if variant not in VARIANTS:
        raise ValueError("variant must be 'cem', 'safe' or 'cost'")
    tr, act = traj, actions
    rows, H1, O = tr.shape
    N, H, A = act.shape

    def pad(a, v):
        a = np.asarray(a, f)
        return np.concatenate([a, np.full(a.shape[:-1] + (128 - O,), v, f)], axis=-1)
    q, g, c, m = pad(tb['q'], 0), pad(ref, 0), pad(tb['c'], 0), pad(tb['goal_mask'], 0)
    if q_terminal is not None:                        # [H + 1, 128]: q on s_0 .. s_{H-1}, q_terminal on s_H
        q = np.concatenate([np.broadcast_to(q, (H, 128)), pad(q_terminal, 0)[None]], axis=0)
    s = np.zeros((rows, H1, 128), f)
    s[..., :O] = tr

    def lane_sum(x, extra=None):                      # [rows, H + 1, 128] -> [rows, H + 1]; extra [rows, H + 1, M]: partial m adds it behind its features
        x = x.reshape(rows, H1, 2, 16, 4)
        acc = np.zeros((rows, H1, 16), f)
        for i in range(2):
            for r in range(4):
                acc = acc + x[:, :, i, :, r]
        if extra is not None:
            acc[..., :extra.shape[-1]] = acc[..., :extra.shape[-1]] + extra
        for _ in range(4):
            acc = acc[..., 0::2] + acc[..., 1::2]
        return acc[..., 0]
    with np.errstate(all='ignore'):
        d = s - g
        dd = d * d
        if ot is None:
            phi = lane_sum(q * dd - c * s)
            nsum = lane_sum(m * dd)
        else:                                         # cem_task_outputs_kernel: output m's terms join partial m of both sums
            y = output_terms(tr, ot)
            e = y - gy
            ee = e * e
            wy = np.broadcast_to(ot['weight'], (H1, y.shape[-1]))
            if q_terminal is not None and ot['terminal'] is not None:
                wy = np.concatenate([wy[:H], ot['terminal'][None]], axis=0)
            phi = lane_sum(q * dd - c * s, wy * ee - ot['linear'] * y)
            nsum = lane_sum(m * dd, ot['near'] * ee)
        r2 = f(task.goal_radius) * f(task.goal_radius)
        near = (nsum <= r2) & bool(r2 > 0) & (variant != 'cost')       # (the cost objective's bytes are not masked by done: near is never true)
        viol = ((tr < tb['lo']) | (tr > tb['hi'])).any(axis=2).astype(f)
        if ot is not None:                            # a bound on an output is a half-space (a NaN compares false)
            viol = ((viol != 0) | ((y < ot['lo']) | (y > ot['hi'])).any(axis=2)).astype(f)
        pen = None
        if zt is not None:                            # cem_task_zones_kernel: a hit is a violation, pen leaves the reward after v
            hit, pen, _ = zone_terms(tr if ot is None else np.concatenate([tr, y], axis=2), zt)
            viol = ((viol != 0) | hit).astype(f)
        u = np.zeros((N, H), f)
        for j in range(A):
            u = u + tb['rho'][j] * (act[:, :, j] * act[:, :, j])
        u = u[np.arange(rows) % N]
        v = rate[np.arange(rows) % N] if rate is not None else None
        clip = f(task.reward_clip) if f(task.reward_clip) > 0 else f(np.inf)
        safe = variant != 'cem'
        cum = np.zeros(rows, f)
        done = np.zeros(rows, bool)
        costs = np.zeros((H, rows), np.uint8) if safe else None
        first = np.full(rows, H, np.int64)
        for t in range(H):
            ga = near[:, t]
            first = np.where(ga & (first == H), t, first)
            r = (-phi[:, t + 1]) - u[:, t]
            if v is not None:
                r = r - v[:, t]
            if pen is not None:
                r = r - pen[:, t + 1]
            r = r + np.where(ga, f(1), f(0)) * f(task.reward_goal)
            r = np.fmin(np.fmax(r, -clip), clip)
            if safe:
                done = done | ga
                nd = np.where(done, f(0), f(1))
                costs[t] = (viol[:, t] * nd).astype(np.uint8)
                cum = cum + r * nd
            else:
                nd = np.where(done, f(0), f(1))
                cum = cum + r * nd
                done = done | ga
    cum = np.ascontiguousarray(cum, f)
    cum.view(np.uint32)[np.isnan(cum)] = np.uint32(0x7fc00000)
    return (cum, costs, first) if return_done else (cum, costs)


def _task_arrays(traj, actions):
    f = np.float32
    tr = np.ascontiguousarray(np.asarray(traj, f))
    act = np.ascontiguousarray(np.asarray(actions, f))
    if tr.ndim != 3 or act.ndim != 3 or tr.shape[1] != act.shape[1] + 1 or tr.shape[0] % act.shape[0] != 0:
        raise ValueError('traj must be [rows, H + 1, O] and actions [N, H, A] with rows a multiple of N')
    if tr.shape[2] > 128:
        raise ValueError('obs_dim > 128')
    return tr, act


def task_objective(traj, actions, task, variant='cem', return_done=False):
    """Host restatement of cem_task_score_kernel (csrc/cem_task_score.h; cem_mpc.h "Task scorers"), bit for bit: traj [rows, H + 1, O]
    raw states, actions [N, H, A] (row r belongs to candidate r mod N), task a QuadraticTask, variant 'cem' | 'safe' | 'cost' ->
    (returns [rows] float32, cost bytes [H, rows] uint8 — None for 'cem', whose rollout stores none).  Every product and sum is a float32
    operation of its own, in the kernel's order: per feature d = s - g, dd = d d, q dd - c s and m dd; sixteen partial sums over the
    features 64 i + 4 l + r (i, then r), added pairwise, neighbours first; u = sum_j rho_j (a_j a_j) from j = 0; the steps in order.
    A NaN return is stored as 0x7fc00000.  return_done=True appends the first step at which near held, int [rows] (H: never)."""
    tr, act = _task_arrays(traj, actions)
    tb = task.tables(tr.shape[2], act.shape[2])
    ot = task.output_tables(tr.shape[2])
    return _task_objective(tr, act, tb, tb['g'], None, None, task, variant, return_done, task.zone_tables(tr.shape[2]), ot,
                           ot['target'] if ot is not None else None)


def tracking_objective(traj, actions, task, variant='cem', k0=0, prev_action=None, return_done=False):
    """Host restatement of cem_task_reference_kernel (csrc/cem_task_reference.h; cem_mpc.h "Tracking tasks"), bit for bit: task_objective
    with task a TrackingTask and the clock (k0, prev_action [A], default zeros).  State s_st is compared with reference row
    min(k0 + st, T - 1); s_H is weighted by terminal_weights; step t also pays v_t = sum_j action_rate_j (e e), e = a_t[j] - a_{t-1}[j]
    (a_{-1} = prev_action), added from j = 0 and subtracted after u: r = ((-phi - u) - v) + bonus."""
    f = np.float32
    tr, act = _task_arrays(traj, actions)
    N, H, A = act.shape
    tb = task.tables(tr.shape[2], A)
    k0 = int(k0)
    if k0 < 0:
        raise ValueError('k0 must be >= 0')
    T = tb['reference'].shape[0]
    ref = tb['reference'][np.minimum(k0 + np.arange(H + 1), T - 1)]
    ap = np.zeros(A, f) if prev_action is None else np.asarray(prev_action, f).reshape(A)
    before = np.concatenate([np.broadcast_to(ap, (N, 1, A)), act[:, :-1]], axis=1)
    with np.errstate(all='ignore'):
        rate = np.zeros((N, H), f)
        for j in range(A):
            e = act[:, :, j] - before[:, :, j]
            rate = rate + tb['action_rate'][j] * (e * e)
    ot = task.output_tables(tr.shape[2])
    gy = None
    if ot is not None:                                # the outputs' reference runs on the same clock (one row: held)
        gy = ot['target'][np.minimum(k0 + np.arange(H + 1), T - 1)] if ot['target'].shape[0] > 1 else ot['target']
    return _task_objective(tr, act, tb, ref, tb['q_terminal'], rate, task, variant, return_done, task.zone_tables(tr.shape[2]), ot, gy)


class PlanReadout(NamedTuple):
    """What a plan knew about the sequence it chose (cem_planner_plan_readout): sequence [H, A] fp32, the best-so-far candidate's whole
    action sequence; score, its score; candidate / iteration, where it was found (-1 / -1: nothing was); particle_returns [P] fp32;
    cost_counts [H] int32, particles with a non-zero cost byte per step (-1: the handle stores no cost bytes); flags (0)."""
    sequence: np.ndarray
    score: np.float32
    candidate: int
    iteration: int
    particle_returns: np.ndarray
    cost_counts: np.ndarray
    flags: int


def empty_readout(horizon, act_dim, particles, has_costs) -> PlanReadout:
    """The block as the tracker's reset leaves it: nothing found."""
    return PlanReadout(np.zeros((int(horizon), int(act_dim)), np.float32), np.float32(-np.inf), -1, -1, np.zeros(int(particles), np.float32),
                       np.full(int(horizon), 0 if has_costs else -1, np.int32), 0)


def track_best(block, it, iters, best_score, scores, elite_idx, actions, ret, costs, n=None) -> PlanReadout:
    """Host restatement of ONE launch of cem_plan_track_kernel (cem_mpc.h, cem_planner_set_plan_readout) — comparisons, copies and integer
    counts, so it is exact.  block: the PlanReadout before the launch; it: the launch's iteration; iters, best_score: ctrl.iters and
    ctrl.best_score as the select in front left them; scores [>= n] as that select ranked them, elite_idx [k] as it stored them;
    actions [>= n, H, A]; ret [P, n] (or flat, P n: the leading part of the workspace array); costs [H, P, n] bytes (or flat), or None on
    handles whose rollout stores none; n: the iteration's population (default: len(scores)).  Returns the block after the launch."""
    it = int(it)
    sc = np.ascontiguousarray(np.asarray(scores, np.float32).reshape(-1))
    n = sc.size if n is None else int(n)
    H, A = block.sequence.shape
    P = block.particle_returns.size
    if it == 0:
        block = empty_readout(H, A, P, costs is not None)
    if int(iters) != it + 1:
        return block
    bs = np.float32(best_score)
    # one fp32 comparison, strict; neither operand is a NaN (keys as the selects rank them: the two zeros tie)
    if not int(score_keys(bs.reshape(1))[0]) > int(score_keys(np.float32(block.score).reshape(1))[0]):
        return block
    e = np.asarray(elite_idx, np.int64).reshape(-1)
    e = np.where((e >= 0) & (e < n), e, 0)                   # (held to the population, as the kernel holds them)
    hit = e[score_keys(sc[e]) == score_keys(bs.reshape(1))[0]]
    if hit.size == 0:
        return block._replace(flags=block.flags | 1)
    c = int(hit.min())
    act = np.asarray(actions, np.float32)
    r = np.asarray(ret, np.float32).reshape(-1)[:P * n].reshape(P, n)
    if costs is None:
        cnt = np.full(H, -1, np.int32)
    else:
        cb = np.asarray(costs, np.uint8).reshape(-1)[:H * P * n].reshape(H, P, n)
        cnt = (cb[:, :, c] != 0).sum(axis=1).astype(np.int32)
    return PlanReadout(np.array(act[c], np.float32, copy=True).reshape(H, A), bs, c, it, np.array(r[:, c], np.float32, copy=True), cnt, block.flags)


def plan_tiles(cfg: PlannerConfig):
    lib = _capi.load()
    cc = to_c_config(cfg)
    rc, nt = C.c_int32(), C.c_int32()
    _capi.check(lib.cem_plan_tiles_host(C.byref(cc), C.byref(rc), C.byref(nt), None, 0), 'cem_plan_tiles_host')
    tiles = np.zeros((nt.value, 6), np.int32)
    _capi.check(lib.cem_plan_tiles_host(C.byref(cc), C.byref(rc), C.byref(nt), _np_ptr(tiles), nt.value), 'cem_plan_tiles_host')
    return rc.value, tiles


def plan_segments(cfg: PlannerConfig):
    """(segments, steps per segment) of the rollout launch this configuration gets (1 segment = unsegmented)."""
    lib = _capi.load()
    cc = to_c_config(cfg)
    ns, sl = C.c_int32(), C.c_int32()
    _capi.check(lib.cem_plan_segments_host(C.byref(cc), C.byref(ns), C.byref(sl)), 'cem_plan_segments_host')
    return ns.value, sl.value


def pack_weights_host(cfg: PlannerConfig, weights) -> np.ndarray:
    lib = _capi.load()
    cc = to_c_config(cfg)
    blob = flatten_weights(weights)
    out = np.zeros(lib.cem_packed_weight_floats(C.byref(cc)), np.float32)
    _capi.check(lib.cem_pack_weights_host(C.byref(cc), _np_ptr(blob), _np_ptr(out)), 'cem_pack_weights_host')
    return out


# ---------------------------------------------------------------------------------------------------------------
# Shape-keyed handle cache: scripts/tune_cem_policy.py replaces agent.policy with fresh CemMpc objects
# of different (H, I, N, k) at run time (reference scripts/tune_cem_policy.py:109-115, "to trigger tensorflow's
# retracing").  A planner handle is this build's "traced graph": one per distinct shape, reused when a shape recurs.
# ---------------------------------------------------------------------------------------------------------------
_PLANNER_CACHE = {}
_PLANNER_CACHE_MAX = 32


def _freeze(v):
    if isinstance(v, np.ndarray) and v.size > 256:      # (a TrackingTask's reference: by its digest)
        return ('ndarray', v.shape, hashlib.sha256(np.ascontiguousarray(v, np.float64).tobytes()).hexdigest())
    if isinstance(v, np.ndarray):
        return tuple(np.asarray(v, np.float64).ravel().tolist())
    if isinstance(v, (list, tuple)):
        return tuple(_freeze(x) for x in v)
    if hasattr(v, '__dataclass_fields__'):
        return tuple((k, _freeze(getattr(v, k))) for k in v.__dataclass_fields__)
    return v


def config_key(cfg: PlannerConfig, device='cuda:0'):
    return (str(device),) + _freeze(cfg)


def cached_planner(cfg: PlannerConfig, device='cuda:0', owner=None, max_batch=None) -> CemPlanner:
    """owner: an object that warm-starts its plans gets a handle of its OWN (the carry lives on the handle, and two users of one handle
    would continue each other's plans): its id joins the key.  None: the handle is shared by everything of this shape.
    max_batch: a batch handle of that capacity (BatchCemPlanner), its own LRU entries in the same cache; None: a single-state handle."""
    key = config_key(cfg, device) + ((('max_batch', int(max_batch)),) if max_batch is not None else ()) + \
        ((('owner', id(owner)),) if owner is not None else ())
    pl = _PLANNER_CACHE.pop(key, None)
    if pl is None:
        pl = CemPlanner(cfg, device=device) if max_batch is None else BatchCemPlanner(cfg, int(max_batch), device=device)
        pl.staged = None                         # (model.uid, model.version) whose weights/normaliser are on the device
        while len(_PLANNER_CACHE) >= _PLANNER_CACHE_MAX:
            # least recently used entry: only the cache's reference goes; a policy still holding the handle keeps it alive
            # (CemPlanner.__del__ destroys it with its last reference)
            _PLANNER_CACHE.pop(next(iter(_PLANNER_CACHE)))
    _PLANNER_CACHE[key] = pl                     # most recently used last
    return pl


def cached_batch_planner(cfg: PlannerConfig, max_batch: int, device='cuda:0', owner=None) -> BatchCemPlanner:
    """cached_planner for batch handles."""
    return cached_planner(cfg, device=device, owner=owner, max_batch=max_batch)


def planner_cache_info():
    return dict(size=len(_PLANNER_CACHE), keys=list(_PLANNER_CACHE.keys()))
