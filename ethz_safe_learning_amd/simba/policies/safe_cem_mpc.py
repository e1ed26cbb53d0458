"""SafeCemMpc, reference simba/policies/safe_cem_mpc.py:7-120: CemMpc whose objective masks done trajectories
before the reward and subtracts 100 from candidates a per-step Beta posterior over particle cost counts calls
unsafe (:76-96,110-120).  Constructor kwargs as :8-19, including the YAML spelling ``posterior_mean_threashold``.

``optimize_for_safety`` (:40-74) is the same CEM loop on the objective ``-compute_mean_costs`` (:98-108), the particle mean of the
cumulative cost, NOT masked by done: a plan that minimises the predicted cost, whatever it earns.  It runs on a planner handle of its
own (``PlannerConfig(variant='cost')``, enum cem_variant CEM_VARIANT_COST) of the policy's shape that shares the model's weights;
``compute_mean_costs`` is that objective as an op on a trajectory tensor and returns the reference's POSITIVE mean costs (the handle's
scores are their negation).  The reference has no caller of either.

Recovery (beyond the reference, off by default): ``recover_below``.  The safe objective has no way out of a state in which every
candidate is deemed unsafe: all scores are shifted by -100 alike and the planner optimises the reward as if nothing were wrong.  With
``recover_below`` a float, a plan whose best score lies below it is followed by ``optimize_for_safety`` on the same state with the same
Philox call number, and THAT action is returned — by ``generate_action``, and for the rows of ``generate_actions`` that fall below it
(re-planned together in one batched cost plan).  ``last_recovered`` says which.  Choosing it: a candidate deemed unsafe scores its
return - 100, so a value such as -50 separates "the best candidate is unsafe" from "it is safe" only when returns are small against
100; with returns of that size no constant does.  It is the caller's number: nothing is claimed here about the returns or the safety of
the resulting agent.  ``None`` (the default, and what every shipped preset has): no cost handle is ever created and every result is bit
for bit what it was.  The cost plans are always cold: warm start (``warm_start=True``) applies to the reward plans alone.

``risk_level`` (CemMpc's, off by default): the reward plans and ``compute_objective`` score a candidate by the mean of its worst particle
returns, and the Beta filter and its -100 apply to that value unchanged.  ``optimize_for_safety``, ``compute_mean_costs`` and the
recovery plans of ``recover_below`` keep running on their cost handle with the particle MEAN of the costs: a tail of the particle costs is
not offered there (cem_mpc.h, cem_planner_set_particle_objective).

Budget-constrained planning (beyond the reference, off by default): ``cost_budget``.  With ``cost_budget`` a float the reward plans rank
candidates by return WITHIN a budget on the predicted cumulative cost instead of by the Beta filter (``PlannerConfig.constraint =
'budget'``, cem_mpc.h CEM_CONSTRAINT_BUDGET): a candidate is feasible when its cost statistic — the particle mean of its
summed, done-masked cost, or with ``cost_risk_level`` in (0, 1] the mean of its ``planner.risk_particles(cost_risk_level, particles)``
WORST particles — is at most the budget; feasible candidates rank by return and, below all of them, infeasible ones by ascending cost.
``posterior_mean_threashold`` then plays no part.  The budget is state of the planner handle, so such a policy plans on handles of its
own (as a warm-started one does); ``set_cost_budget`` changes it between decisions without re-capturing anything — to lower it as an
episode's costs accrue, or, with an array, to give the rows of ``generate_actions`` budgets of their own.  After a plan
``last_feasible`` says whether the best candidate was feasible (a bool, or a bool array over the rows) and ``last_cost_total`` holds the
summed cost T that ranked an infeasible best (``None`` where it is feasible).  An infeasible best scores below -2^100, hence below any
``recover_below``, which keeps working unchanged and replaces it by the ``optimize_for_safety`` action.  ``optimize_for_safety`` and
``compute_mean_costs`` are untouched.  ``None`` (the default, and what every shipped preset has) touches no handle and changes no bit.
Nothing is claimed about the returns or the safety of an agent that uses it.

``noise_beta`` / ``noise_rho`` (CemMpc's, off by default): the reward plans sample time-correlated action sequences, and so do
``optimize_for_safety`` and the recovery plans of ``recover_below`` — the cost handle is the policy's configuration with another
objective, the sampler is shared and there is no reason for it to differ.

``keep_elites`` / ``shift_elites`` (CemMpc's, off by default): the reward plans carry elites over as CemMpc's do.  ``optimize_for_safety``
and the recovery plans of ``recover_below`` carry them from iteration to iteration only: their handle is shared through the cache and
their plans follow no earlier cost plan.

``population_decay`` / ``min_population`` / ``mean_candidate`` (CemMpc's, off by default): the reward plans, ``optimize_for_safety`` and the
recovery plans of ``recover_below`` all follow the policy's setting; ``generate_actions`` is refused as CemMpc's is.

``plan_readout`` / ``replan_every`` (CemMpc's, off by default): the cost handle gets the read-out too, and when ``recover_below`` replaces
a plan by ``optimize_for_safety`` — in ``generate_action`` and for the replaced rows of ``generate_actions`` — ``last_plan`` /
``last_plans`` and the sequence kept for ``replan_every`` are those of the plan whose action is returned, the cost plan's.  On the cost
handle ``score`` is minus the mean un-masked cumulative cost and ``cost_counts`` count the non-zero ones among the cost bytes that
score sums (cem_score.h, cem_constraint_reduce_kernel); ``particle_returns`` hold what the rollout leaves in ``ret`` there — the done-masked
returns of the safe objective's launch, which the cost objective never reads: they describe the candidate, not its score."""
import dataclasses

import numpy as np

from ...planner import cached_batch_planner, cached_planner, decode_constrained_score, risk_particles
from .cem_mpc import CemMpc


class SafeCemMpc(CemMpc):
    variant = 'safe'

    def __init__(self, model, environment, horizon, iterations, smoothing, n_samples, n_elite, particles,
                 stddev_threshold, noise_stddev, posterior_mean_threashold, recover_below=None, cost_budget=None, cost_risk_level=None,
                 **kwargs):
        super().__init__(model, environment, horizon, iterations, smoothing, n_samples, n_elite, particles,
                         stddev_threshold, noise_stddev, **kwargs)
        self.cost = getattr(environment, 'get_cost', None)
        self.posterior_mean_threashold = posterior_mean_threashold
        self.recover_below = None if recover_below is None else float(recover_below)
        self._cost_planner = None                      # the CEM_VARIANT_COST handle of optimize_for_safety, built on first use
        self._cost_batch_planners = {}                 # capacity (a power of two) -> cost batch handle (recovery in generate_actions)
        self.last_safety_score = None                  # best score of the last optimize_for_safety: minus its mean cost
        self.last_recovered = None                     # bool (generate_action) / bool [B] (generate_actions): the action is a recovery plan's
        # budget-constrained planning (beyond the reference's kwargs): see the module docstring
        if cost_budget is None and cost_risk_level is not None:
            raise ValueError('cost_risk_level needs a cost_budget')
        self.cost_budget = None if cost_budget is None else self._as_budget(cost_budget)
        self.cost_risk_level = None if cost_risk_level is None else float(cost_risk_level)
        self.worst_cost_particles = 0 if cost_risk_level is None else risk_particles(cost_risk_level, particles)
        self._objective_budget_planner = None          # compute_objective's own minimal handle while the planning handle is not built
        self.last_feasible = None                      # bool (generate_action) / bool [B] (generate_actions): the best candidate met the budget
        self.last_cost_total = None                    # the summed cost T of an infeasible best, None where it is feasible (per row: an object array)

    def _extra_config(self):
        if self.cost_budget is None:
            return dict(posterior_mean_threashold=self.posterior_mean_threashold)
        return dict(posterior_mean_threashold=self.posterior_mean_threashold, constraint='budget', worst_cost_particles=self.worst_cost_particles)

    # ---- the cost budget ------------------------------------------------------------------------------
    @staticmethod
    def _as_budget(value):
        b = np.asarray(value, np.float32)
        if b.ndim > 1 or b.size < 1 or np.isnan(b).any():
            raise ValueError('cost_budget is a float or one float per row, not NaN')
        return np.float32(b) if b.ndim == 0 else b.copy()

    def set_cost_budget(self, value):
        """The budget of the following plans: a float, or an array with one budget per row of the following generate_actions calls.
        A stream-ordered copy on the policy's own handles; nothing is re-captured."""
        if self.cost_budget is None:
            raise ValueError('this policy was built without a cost budget (the constraint is part of its handles\' configuration): '
                             'construct it with cost_budget=')
        self.cost_budget = self._as_budget(value)

    def _owns_handles(self):
        return super()._owns_handles() or self.cost_budget is not None

    def _stage_budget(self, planner, scalar_only=False):
        """The policy's budget onto one of its handles, when it is not what the handle holds already."""
        b = self.cost_budget
        if np.ndim(b) and (scalar_only or b.size > planner.max_batch):
            raise ValueError('%d budgets for a handle of %d problem row(s)' % (b.size, planner.max_batch))
        tag = np.atleast_1d(b).tobytes() + bytes([np.ndim(b)])
        if getattr(planner, 'budget_staged', None) != tag:
            planner.set_cost_budget(b)
            planner.budget_staged = tag

    def build(self):
        super().build()
        if self.cost_budget is not None:
            self._stage_budget(self._planner, scalar_only=True)

    def build_batch(self, n):
        pl = super().build_batch(n)
        if self.cost_budget is not None:
            self._stage_budget(pl)
        return pl

    def _objective_planner(self, variant=None):
        if variant is not None or self.cost_budget is None:
            return super()._objective_planner(variant)
        pl = self._planner
        if pl is None or pl.h is None:                 # not built: a minimal handle of the policy's own carries the constraint and the budget
            pl = self._objective_budget_planner
            if pl is None or pl.h is None:
                cfg = dataclasses.replace(self._objective_config(), constraint='budget', worst_cost_particles=self.worst_cost_particles)
                pl = self._objective_budget_planner = cached_planner(cfg, device=self.device, owner=self)
        self._stage_budget(pl, scalar_only=True)
        return pl

    def _note_feasibility(self, scores):
        """last_feasible / last_cost_total from the best score(s) of the plan just made."""
        if self.cost_budget is None:
            return
        dec = [decode_constrained_score(s) for s in np.atleast_1d(scores)]
        if np.ndim(scores) == 0:
            self.last_feasible, self.last_cost_total = dec[0]
        else:
            self.last_feasible = np.array([f for f, _ in dec], bool)
            self.last_cost_total = np.array([t for _, t in dec], object)

    def _objective_extra_config(self):
        return dict(posterior_mean_threashold=self.posterior_mean_threashold)

    # ---- the cost objective (safe_cem_mpc.py:40-74,98-108) --------------------------------------------------------
    def cost_planner_config(self):
        return dataclasses.replace(self.planner_config(), variant='cost', worst_particles=0,      # (the cost objective has no lower tail
                                   constraint='beta', worst_cost_particles=0,                     # and no budget;
                                   refit='uniform', refit_temperature=0.0,                        # recovery plans keep the uniform refit;
                                   shift_elites=False, elite_shift=1)                             # they carry elites within a plan only;
                                                                                                  # the action noise stays the policy's)

    def build_cost(self):
        """The cost handle of the policy's shape (shared through the cache like the planning handle), the model's weights staged."""
        if self._cost_planner is None or self._cost_planner.h is None:
            self._cost_planner = cached_planner(self.cost_planner_config(), device=self.device)
        self._sync_model(self._cost_planner)
        return self._cost_planner

    def build_cost_batch(self, n):
        cap = 1 << max(int(n) - 1, 0).bit_length()
        pl = self._cost_batch_planners.get(cap)
        if pl is None or pl.h is None:
            pl = self._cost_batch_planners[cap] = cached_batch_planner(self.cost_planner_config(), cap, device=self.device)
        self._sync_model(pl)
        return pl

    def optimize_for_safety(self, state, call=None):
        """safe_cem_mpc.py:40-74: state[O] -> np.float32[A], ``best_so_far + noise`` of the CEM loop that maximises minus the mean
        cost (no score is returned, as :74; it is kept in ``last_safety_score``).  call: the Philox call number (None: the cost
        handle's own counter)."""
        cpl = self.build_cost()
        self._stage_clock(cpl)                         # (a TrackingTask: the recovery plan follows the same reference from the same step)
        action, score, _ = cpl.plan(np.asarray(state, np.float32), seed=self.seed, call=call)
        self.last_safety_score = score
        return action

    def compute_mean_costs(self, trajectories, action_sequences=None):
        """safe_cem_mpc.py:98-108: trajectories [particles*n, H+1, obs] (rows p*n + candidate) -> the mean over particles of every
        candidate's summed, un-masked cost, [n], >= 0.  ``action_sequences`` is accepted for signature parity (get_cost ignores
        actions).  numpy in -> numpy out, torch in -> torch (GPU) out."""
        pl = self._cost_planner if self._cost_planner is not None and self._cost_planner.h is not None else self._objective_planner('cost')
        costs = -pl.compute_objective(trajectories)           # the handle's scores are minus the mean cost (cem_mpc.h)
        return costs.cpu().numpy() if isinstance(trajectories, np.ndarray) else costs

    # ---- opt-in recovery ------------------------------------------------------------------------------------------
    def generate_action(self, state):
        if self.recover_below is None or self._kept is not None:      # (a decision between two plans follows the plan in force, whichever it was)
            action = super().generate_action(state)
            self._note_feasibility(self.last_score)
            return action
        self.build()
        call = self._next_calls([self.slot])[0] if self.warm_start else int(self._planner.take_calls()[0])
        state = np.asarray(state, np.float32)
        self._stage_clock(self._planner)
        action, score, iters = self._planner.plan(state, seed=self.seed, call=call)
        self.last_score, self.last_iterations = score, iters
        self._note_ess(self._planner, iters)
        self._note_feasibility(score)
        self.last_recovered = bool(score < self.recover_below)
        if self.last_recovered:
            action = self.optimize_for_safety(state, call=call)
        self._note_plan(self._cost_planner if self.last_recovered else self._planner)
        return self._note_decision(action)

    def generate_actions(self, states, slots=None, reset=None):
        if self.cost_budget is not None and np.ndim(self.cost_budget) and self.cost_budget.size != np.shape(states)[0]:
            raise ValueError('%d budgets for %d rows of states' % (self.cost_budget.size, np.shape(states)[0]))
        actions = super().generate_actions(states, slots=slots, reset=reset)
        self._note_feasibility(np.asarray(self.last_scores))
        if self.recover_below is None:
            return actions
        self.last_recovered = np.asarray(self.last_scores) < self.recover_below
        rows = np.nonzero(self.last_recovered)[0]
        if rows.size:                                   # the rows below the threshold, together, with the call numbers of the plans they replace
            st = np.asarray(states, np.float32)
            cpl = self.build_cost_batch(rows.size)
            actions[rows], _, _ = cpl.plan_batch(st[rows], seed=self.seed, calls=np.asarray(self.last_calls, np.uint64)[rows])
            if self.plan_readout:
                for j, b in enumerate(rows):
                    self.last_plans[int(b)] = cpl.plan_readout(j)
        return actions
