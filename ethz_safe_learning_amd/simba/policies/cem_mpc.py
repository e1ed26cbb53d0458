"""CemMpc, reference simba/policies/cem_mpc.py:6-68, on the HIP planner.

Same constructor kwargs (cem_mpc.py:7-17), same ``generate_action(state) -> np.float32[A]`` contract
(cem_mpc.py:31-33; caller simba/agents/agent.py:120).  One ``CemPlanner`` handle corresponds to the reference's one
traced ``@tf.function`` graph; it is built lazily on the first call and rebuilt never (a shape change is a new
policy object, as in scripts/tune_cem_policy.py:109-115).  Weights / normaliser are re-staged whenever the model's
``version`` changed (after ``fit``: mbrl_agent.py:53).

Warm start (beyond the reference, off by default): with ``warm_start=True`` every plan starts from the previous plan's distribution
shifted ``warm_shift`` steps (planner.CemPlanner.set_warm_start) instead of the action box; ``reset()`` — called by the agent at every
episode start — makes the next plan a cold one again.  The carry lives on the planner handle, and handles are shared between policy
objects of one shape; a warm-started policy therefore gets handles of its OWN (``owner=`` of cached_planner / cached_batch_planner),
so two policies of one shape never continue each other's plans.
A warm-started policy also numbers its plans per ENVIRONMENT: the Philox call number of environment e's d-th decision is
``e * 2**32 + d``, whether the decision is planned alone (``generate_action``, environment ``self.slot``, 0 by default) or as a row of
``generate_actions(..., slots=)`` — so an environment sees the same plans however it is batched with others.

Risk-averse planning (beyond the reference, off by default): with ``risk_level`` a float in (0, 1] a candidate's score is the mean of
the ``m = planner.risk_particles(risk_level, particles)`` SMALLEST of its particle returns (CVaR at level m / particles;
``PlannerConfig.worst_particles``, cem_mpc.h CEM_PARTICLES_LOWER_TAIL) instead of the mean of all of them: ``generate_action``,
``generate_actions`` and ``compute_objective`` then run on that lower tail.  ``None`` (the default, and what every shipped preset has)
changes no handle and no bit.  Nothing is claimed about the returns or the safety of an agent that uses it.

Score-weighted refit (beyond the reference, off by default): with ``elite_temperature`` a float > 0 an iteration refits mu and sigma
from the elites weighted by ``exp((score - best elite score) / elite_temperature)`` instead of 1 / n_elite each
(``PlannerConfig.refit = 'softmax'``, cem_mpc.h CEM_REFIT_SOFTMAX): MPPI's update when n_elite = n_samples, "weighted
elites" below that.  ``generate_action``, ``generate_actions`` and warm-started plans use it; ``last_ess`` holds the effective sample
size of every iteration of the last plan (a float array; one per row after ``generate_actions``), each in [1, n_elite].  ``None`` (the
default, and what every shipped preset has) changes no handle and no bit.  Nothing is claimed about the returns or the safety of an
agent that uses it.

Time-correlated action noise (beyond the reference, off by default): with ``noise_beta`` a float >= 0 the sampler draws every action
sequence from power-law noise of that spectral exponent (planner.powerlaw_mixing: 1 pink, 2 red; periodic in the horizon, like iCEM's
FFT sampler), with ``noise_rho`` a float in (-1, 1) from AR(1) noise of that lag-1 correlation (planner.ar1_mixing: no wrap-around) —
``PlannerConfig.action_noise``, cem_mpc.h CEM_NOISE_MIXED; DESIGN.md 4.11 — instead of drawing every step independently, so that a
candidate holds a direction for several steps.  Give at most one of the two.  ``generate_action``, ``generate_actions`` and warm-started
plans use it; the plan then runs the generic rollout kernels (the lean ones draw in place).  ``None`` for both (the default, and what
every shipped preset has) touches no handle and changes no bit.  Nothing is claimed about the returns or the safety of an agent that
uses it.

Elite carry-over (beyond the reference, off by default): with ``keep_elites`` a fraction in (0, 1] of ``n_elite`` (iCEM uses 0.3) the best
``planner.elite_keep_count(keep_elites, n_elite)`` elites of an iteration are candidates of the next one, rolled out and scored again
(``PlannerConfig.keep_elites``, cem_mpc.h cem_planner_set_elite_carry) instead of surviving as moments only.
``generate_action``, ``generate_actions`` and warm-started plans use it; the plan then samples in a launch of its own and runs the generic
rollout kernels.  With ``shift_elites=True`` (which requires ``keep_elites``) the first iteration of a plan also takes the previous plan's
last kept elites, moved ``warm_shift`` steps towards the present, the freed tail drawn anew: the store lives on the planner handle, so
such a policy plans on handles of its OWN (as a warm-started one does), ``reset()`` empties it, and ``generate_actions`` is refused with
a ``ValueError`` — a batch handle's rows move between slots and carry nothing across plans.  ``None`` / ``False`` (the defaults, and what
every shipped preset has) touch no handle and change no bit.  Nothing is claimed about the returns or the safety of an agent that uses
it.

Population decay and the mean candidate (beyond the reference, off by default): with ``population_decay`` a float >= 1 (iCEM uses 1.25)
iteration i samples ``planner.population_schedule(n_samples, n_elite, iterations, population_decay, particles, ensemble_size,
min_population)[i]`` candidates instead of ``n_samples`` — about ``n_samples / population_decay**i``, not below ``min_population``
(default ``2 * n_elite``) — each iteration launched as a plan of that population would launch it (``PlannerConfig.population``, cem_mpc.h
cem_planner_set_population_schedule): the one iCEM ingredient that saves work.  With ``mean_candidate=True`` the last
candidate of the last iteration is the clipped mean itself (``PlannerConfig.mean_candidate``).  ``generate_action`` and warm-started
plans use both; ``generate_actions`` is refused with a ``ValueError`` — a batch handle launches the tiles of ONE plan for all its rows.
``None`` / ``False`` (the defaults, and what every shipped preset has) touch no handle and change no bit.  Nothing is claimed about the
returns or the safety of an agent that uses them.

Plan read-out and open-loop steps (beyond the reference, off by default): with ``plan_readout=True`` a tracker kernel behind every
select keeps what the plan knew about its choice (``PlannerConfig.plan_readout``, cem_mpc.h cem_planner_set_plan_readout; DESIGN.md
4.14) and ``last_plan`` holds it after every ``generate_action`` as a ``planner.PlanReadout``: the whole best action sequence
``sequence [H, A]``, its ``score``, the ``candidate`` and ``iteration`` that found it, the candidate's ``particle_returns [P]`` and, on
the safe variant, ``cost_counts [H]`` — how many of the P particles predicted a cost at each step of the plan.  After
``generate_actions`` ``last_plans`` holds one per row.  ``generate_action_sequence(state)`` plans and returns ``last_plan.sequence``.
Sampler, rollout, select and refit launch as before (the lean rollout stays); every read of the block waits for the planner's stream.
Task scorers (beyond the reference, off by default): with ``task=planner.QuadraticTask(...)`` rollouts are scored by a quadratic reward
with box state constraints instead of the Safety-Gym scorer (``PlannerConfig.task``, cem_mpc.h cem_planner_set_task):
the policy then plans for environments whose observation is no lidar vector, and the environment need not expose a scorer.  Every
option above applies; ``generate_actions`` raises (batch handles do not serve a task).
With ``task=planner.TrackingTask(...)`` the set-point is a reference table that moves with time, the last predicted state has weights of
its own and the change of the action is penalised (cem_mpc.h cem_planner_set_task_tracking).  The policy keeps the
handle's clock: before every plan it sets it to (decisions since ``reset()``, the action it returned last) with a stream-ordered copy
(the captured graph stays); the decisions between two plans of ``replan_every`` advance the count too; ``reset()`` puts back (0, zeros).
Either task may carry ``zones=planner.StateZones(...)``: round regions of the state space the plan must stay out of (or inside of) — a
state that hits one is a cost exactly as a state outside the box is, so ``SafeCemMpc``'s filter, budget, recovery and ``last_plan``'s
cost counts see it, and coming within ``margin`` of one costs reward (cem_mpc.h cem_planner_set_task_zones).
Either task may also carry ``outputs=planner.TaskOutputs(...)``: up to 16 linear outputs y = C s with a feature's vocabulary each — a
full-matrix cost (``TaskOutputs.quadratic_form``), half-spaces (``TaskOutputs.halfspaces``: a bound that is crossed is a cost as above),
and zone axes ``obs_dim + m`` for rotated zones (cem_mpc.h cem_planner_set_task_outputs).

With ``replan_every=r``, 1 <= r <= horizon (which implies ``plan_readout``), ``generate_action`` plans at decisions 0, r, 2r, ... of an
episode and in between returns step j of the kept sequence, plus ``noise_stddev`` times the output noise of that decision's own Philox
call number (no draw, and an exact copy, when ``noise_stddev`` is 0): every decision consumes one call number, ``last_score`` /
``last_iterations`` / ``last_plan`` stay those of the plan in force, ``reset()`` discards the kept sequence so that the next decision
plans.  With ``warm_start`` or ``shift_elites`` the carried distribution and elites move ``warm_shift`` steps per plan, so ``warm_shift``
must equal ``replan_every``; ``generate_actions`` is refused with ``replan_every > 1`` (no per-row sequences on batch handles).
``False`` / 1 (the defaults, and what every shipped preset has) touch no handle and change no bit.  Nothing is claimed about the
returns or the safety of an agent that uses them."""
import logging
import numpy as np

from ...planner import PlannerConfig, ScorerConfig, TrackingTask, cached_batch_planner, cached_planner, elite_keep_count, population_schedule, risk_particles, stage_model_weights
from .mpc_policy import MpcPolicy


class CemMpc(MpcPolicy):
    variant = 'cem'

    def __init__(self, model, environment, horizon, iterations, smoothing, n_samples, n_elite, particles,
                 stddev_threshold, noise_stddev, seed=0, device='cuda:0', use_graph=True, precision='fp32',
                 warm_start=False, warm_shift=1, warm_tail='box', warm_sigma='reset', warm_sigma_floor=0.25, risk_level=None,
                 elite_temperature=None, noise_beta=None, noise_rho=None, keep_elites=None, shift_elites=False,
                 population_decay=None, min_population=None, mean_candidate=False, plan_readout=False, replan_every=1, task=None):
        super().__init__(model, environment, horizon, n_samples, particles)
        # a task scorer (beyond the reference's kwargs): see the module docstring
        self.task = task
        self._clock = (0, None)                        # a TrackingTask's clock: decisions since reset(), the action returned last (None: zeros)
        self.iterations = iterations
        self.smoothing = smoothing
        self.elite = n_elite
        self.stddev_threshold = stddev_threshold
        self.noise_stddev = noise_stddev
        self.seed = seed
        self.device = device
        self.use_graph = use_graph
        self.precision = precision                     # 'fp32' | 'bf16x3' (fp32-grade) | 'bf16' (reduced precision: dense operands rounded to
                                                       # bf16) — PlannerConfig.precision; beyond the reference's kwargs
        # warm start (beyond the reference's kwargs, like precision): see the module docstring
        self.warm_start, self.warm_shift, self.warm_tail, self.warm_sigma, self.warm_sigma_floor = bool(warm_start), warm_shift, warm_tail, warm_sigma, warm_sigma_floor
        # risk-averse planning (beyond the reference's kwargs): see the module docstring
        self.risk_level = None if risk_level is None else float(risk_level)
        self.worst_particles = 0 if risk_level is None else risk_particles(risk_level, particles)
        # score-weighted refit (beyond the reference's kwargs): see the module docstring
        self.elite_temperature = None if elite_temperature is None else float(elite_temperature)
        if self.elite_temperature is not None and not (np.isfinite(self.elite_temperature) and self.elite_temperature > 0.0):
            raise ValueError('elite_temperature must be finite and > 0, got %r' % (elite_temperature,))
        # time-correlated action noise (beyond the reference's kwargs): see the module docstring
        if noise_beta is not None and noise_rho is not None:
            raise ValueError('give at most one of noise_beta and noise_rho')
        self.noise_beta = None if noise_beta is None else float(noise_beta)
        self.noise_rho = None if noise_rho is None else float(noise_rho)
        if self.noise_beta is not None and not (np.isfinite(self.noise_beta) and self.noise_beta >= 0.0):
            raise ValueError('noise_beta must be finite and >= 0, got %r' % (noise_beta,))
        if self.noise_rho is not None and not -1.0 < self.noise_rho < 1.0:
            raise ValueError('noise_rho must lie in (-1, 1), got %r' % (noise_rho,))
        # elite carry-over (beyond the reference's kwargs): see the module docstring
        self.keep_elites = None if keep_elites is None else float(keep_elites)
        self.n_keep = 0 if keep_elites is None else elite_keep_count(keep_elites, n_elite)
        self.shift_elites = bool(shift_elites)
        if self.shift_elites and self.keep_elites is None:
            raise ValueError('shift_elites needs keep_elites')
        # population decay and the mean candidate (beyond the reference's kwargs): see the module docstring
        self.population_decay = None if population_decay is None else float(population_decay)
        self.min_population = None if min_population is None else int(min_population)
        if self.population_decay is None and self.min_population is not None:
            raise ValueError('min_population needs population_decay')
        if self.population_decay is not None and not (np.isfinite(self.population_decay) and self.population_decay >= 1.0):
            raise ValueError('population_decay must be finite and >= 1, got %r' % (population_decay,))
        self.mean_candidate = bool(mean_candidate)
        # plan read-out and open-loop steps (beyond the reference's kwargs): see the module docstring
        self.replan_every = int(replan_every)
        if self.replan_every != replan_every or not 1 <= self.replan_every <= int(horizon):
            raise ValueError('replan_every must be an integer in [1, horizon = %d], got %r' % (int(horizon), replan_every))
        if self.replan_every > 1 and (self.warm_start or self.shift_elites) and int(warm_shift) != self.replan_every:
            raise ValueError('replan_every = %d executes %d steps between two plans, but warm_start / shift_elites move the carried distribution '
                             'and elites warm_shift = %r steps: the two must be equal' % (self.replan_every, self.replan_every, warm_shift))
        self.plan_readout = bool(plan_readout) or self.replan_every > 1
        self.last_plan = None                          # planner.PlanReadout of the plan in force (plan_readout)
        self.last_plans = None                         # ... one per row of the last generate_actions
        self._kept = None                              # replan_every: the sequence being executed open loop,
        self._kept_step = 0                            # and the step of it the next decision returns
        self.last_ess = None                           # ESS per iteration of the last weighted plan (generate_actions: a list, one array per row)
        self._warm_token = object()                    # marks the handles this policy has configured (ids are reused after garbage collection)
        self._warm_cap = 1                             # slots the warm-started batch handle must hold
        self.slot = 0                                  # the environment generate_action plans for (warm start: its call numbers)
        self._decisions = {}                           # environment -> decisions planned so far (warm start: call numbering)
        self._planner = None
        self._batch_planners = {}                      # capacity (a power of two) -> batch handle (generate_actions)
        self.last_score = None
        self.last_iterations = None
        self.last_scores = None
        self.last_calls = None                         # Philox call numbers of the rows of the last generate_actions

    # ---- planner plumbing -------------------------------------------------------------------------------------
    def _extra_config(self):
        return {}

    def _refit_config(self):
        if self.elite_temperature is None:
            return {}
        return dict(refit='softmax', refit_temperature=self.elite_temperature)

    def _noise_config(self):
        if self.noise_beta is not None:
            return dict(action_noise='powerlaw', action_noise_param=self.noise_beta)
        if self.noise_rho is not None:
            return dict(action_noise='ar1', action_noise_param=self.noise_rho)
        return {}

    def _carry_config(self):
        if not self.n_keep:
            return {}
        return dict(keep_elites=self.n_keep, shift_elites=self.shift_elites, elite_shift=self.warm_shift if self.shift_elites else 1)

    def _population_config(self):
        out = {}
        if self.population_decay is not None:
            sched = population_schedule(self.n_samples, self.elite, self.iterations, self.population_decay, self.particles,
                                        self.model.model.ensemble_size, self.min_population)
            if any(n != self.n_samples for n in sched):
                out['population'] = tuple(sched)
        if self.mean_candidate:
            out['mean_candidate'] = True
        return out

    def _readout_config(self):
        return dict(plan_readout=True) if self.plan_readout else {}

    def _task_config(self):
        return dict(task=self.task) if self.task is not None else {}

    def _scorer_config(self):
        scorer = getattr(self.environment, '_scorer', None) or getattr(self.environment, 'scorer', None)
        if scorer is None and self.task is not None:      # a task plan never reads the Safety-Gym scorer: any valid one serves
            return ScorerConfig(goal_slice=(0, 1))
        if scorer is None:
            raise ValueError('environment must expose its SafetyGymStateScorer as `_scorer` (as MbrlSafetyGym does, '
                             'reference simba/environment_utils/safety_gym.py:27-29)')
        return scorer.to_scorer_config()

    def planner_config(self):
        m = self.model
        ens = m.model
        return PlannerConfig(
            obs_dim=m.observation_space_dim, act_dim=m.action_space_dim, ensemble_size=ens.ensemble_size,
            particles=self.particles, n_samples=self.n_samples, horizon=self.horizon, n_elite=self.elite,
            iterations=self.iterations, scorer=self._scorer_config(), act_low=self.action_space.low,
            act_high=self.action_space.high, units=ens.mlp_params['units'], n_layers=ens.mlp_params['n_layers'], activation=ens.activation,
            smoothing=self.smoothing, stddev_threshold=self.stddev_threshold, noise_stddev=self.noise_stddev,
            variant=self.variant, sampling_propagation=m.sampling_propagation, scale_features=m.scale_features,
            use_graph=self.use_graph, precision=self.precision, worst_particles=self.worst_particles, **self._refit_config(),
            **self._noise_config(), **self._carry_config(), **self._population_config(), **self._readout_config(),
            **self._task_config(), **self._extra_config())

    def _owns_handles(self):
        """Whether this policy's planning handles carry state of its own (the warm-start carry, the elites kept across plans; SafeCemMpc:
        a cost budget) and so must not be shared through the cache with other policies of the shape."""
        return self.warm_start or self.shift_elites

    def build(self):
        if self._planner is None or self._planner.h is None:      # never built, or closed by its owner
            # one handle per distinct shape, shared by every policy object of that shape (tune_cem_policy.py:109-115)
            self._planner = self._own(cached_planner(self.planner_config(), device=self.device, owner=self if self._owns_handles() else None))
        self._sync_model()

    def _sync_model(self, planner=None):
        planner = self._planner if planner is None else planner
        tag = (self.model.uid, self.model.version)            # uid, not id(): ids are reused after garbage collection
        if planner.staged != tag:
            stage_model_weights(planner, self.model.model)
            planner.set_normaliser(self.model.inputs_min, self.model.inputs_max)
            planner.staged = tag

    def _own(self, planner):
        """A handle fresh from the cache: with warm start on, make it this policy's (shift mode on every slot, no carry); with elites kept
        across plans, empty its stores."""
        if (self.warm_start or self.shift_elites) and getattr(planner, 'warm_owner', None) is not self._warm_token:
            if self.warm_start:
                planner.set_warm_start(shift=self.warm_shift, tail=self.warm_tail, sigma=self.warm_sigma, floor_frac=self.warm_sigma_floor)
                planner.set_init_mode('shift', slot=None)
            planner.reset_carry()
            planner.warm_owner = self._warm_token
        return planner

    def reset(self):
        """An episode begins: the next plan of every slot starts cold and takes no elites of an earlier plan (no effect without warm
        start or shift_elites), and the sequence kept for replan_every is discarded."""
        self._kept, self._kept_step = None, 0          # replan_every: the next decision plans
        self._clock = (0, None)
        if not (self.warm_start or self.shift_elites):
            return
        for pl in [self._planner] + list(self._batch_planners.values()):
            if pl is not None and pl.h is not None:
                pl.reset_carry()

    def build_batch(self, n):
        """The batch handle for n observations: capacity n rounded up to a power of two (one cached handle, hence one captured
        graph, per capacity), with the current model version's weights / normaliser staged."""
        if self.warm_start:
            # ONE handle holds every environment's carry: its capacity never shrinks with the number of rows (a larger one starts cold)
            n = self._warm_cap = max(int(n), self._warm_cap)
            grown = [c for c in self._batch_planners if c < (1 << max(n - 1, 0).bit_length())]
            for c in grown:                            # more environments than the handle in use holds: a larger one takes over, cold
                logging.getLogger(__name__).warning('warm start: %d environments exceed the batch handle of %d slots; a larger handle '
                                                    'takes over and every environment\'s next plan starts cold', n, c)
                del self._batch_planners[c]
        cap = 1 << max(int(n) - 1, 0).bit_length()
        pl = self._batch_planners.get(cap)
        if pl is None or pl.h is None:
            pl = self._batch_planners[cap] = self._own(cached_batch_planner(self.planner_config(), cap, device=self.device,
                                                                            owner=self if self._owns_handles() else None))
        self._sync_model(pl)
        return pl

    def _stage_clock(self, planner):
        """A TrackingTask's clock onto the handle about to plan (handles are shared through the cache: every plan sets its own)."""
        if isinstance(self.task, TrackingTask):
            k0, prev = self._clock
            planner.set_task_clock(k0, np.zeros(planner.cfg.act_dim, np.float32) if prev is None else prev)

    def _note_decision(self, action):
        """The decision just made moves the clock on: one more step into the reference, `action` the one before the next plan's first."""
        if isinstance(self.task, TrackingTask):
            self._clock = (self._clock[0] + 1, np.array(action, np.float32, copy=True))
        return action

    # ---- the plugin boundary ------------------------------------------------------------------------------------
    def generate_action(self, state):
        self.build()                                   # cached handle + weights of the current model version
        if self._kept is not None:                     # replan_every: a decision between two plans
            return self._note_decision(self._follow(self._next_calls([self.slot])[0] if self.warm_start else int(self._planner.take_calls()[0])))
        self._stage_clock(self._planner)
        action, score, iters = self._planner.plan(np.asarray(state, np.float32), seed=self.seed,
                                                  call=self._next_calls([self.slot])[0] if self.warm_start else None)
        self.last_score, self.last_iterations = score, iters
        self._note_ess(self._planner, iters)
        self._note_plan(self._planner)
        return self._note_decision(action)

    def _note_plan(self, planner):
        """last_plan from the handle whose action is being returned (its stream is drained: the last tracker runs behind the polled
        result), and with replan_every the sequence the next decisions follow."""
        if not self.plan_readout:
            return
        self.last_plan = planner.plan_readout(0)
        if self.replan_every > 1:
            self._kept, self._kept_step = self.last_plan.sequence, 1

    def _follow(self, call):
        """Step _kept_step of the kept sequence as the decision numbered `call`: plus that call's output noise where the policy adds any."""
        action = np.array(self._kept[self._kept_step], np.float32, copy=True)
        if self.noise_stddev != 0:
            action = action + self._planner.output_noise(self.seed, call) * np.float32(self.noise_stddev)
        self._kept_step += 1
        if self._kept_step >= self.replan_every:
            self._kept, self._kept_step = None, 0
        return action

    def generate_action_sequence(self, state):
        """Plan for `state` and return the whole best action sequence, np.float32 [H, A] (last_plan.sequence): sequence[0] is the
        planned action before the output noise.  Needs plan_readout=True."""
        if not self.plan_readout:
            raise ValueError('generate_action_sequence needs plan_readout=True (or replan_every > 1)')
        self._kept, self._kept_step = None, 0          # (a plan, whatever was being followed)
        self.generate_action(state)
        return self.last_plan.sequence

    def _note_ess(self, planner, iters):
        """last_ess from the handle that has just planned (iters: an int, or one per row of a batched plan)."""
        if self.elite_temperature is None:
            return
        if np.ndim(iters) == 0:
            self.last_ess = planner.refit_stats(0, n=max(int(iters), 1))
        else:
            self.last_ess = [planner.refit_stats(b, n=max(int(i), 1)) for b, i in enumerate(iters)]

    def _next_calls(self, slots):
        """Call numbers of the next decision of every environment in `slots` (module docstring), counted."""
        out = []
        for e in slots:
            d = self._decisions.get(int(e), 0)
            self._decisions[int(e)] = d + 1
            out.append((int(e) << 32) + d)
        return out

    accepts_slots = True                               # generate_actions takes slots / reset (BaseAgent.sample_trajectories_lockstep)

    def generate_actions(self, states, slots=None, reset=None):
        """generate_action for every row of states[B, O] in ONE batched plan -> np.float32[B, A]: row b is what generate_action
        returns for states[b] with the same call number (BatchCemPlanner.plan_batch).  Sets last_scores / last_iterations (arrays).
        Warm start: slots[B] is the environment index of every row (distinct; default: the row index) — row b continues the plans of
        ITS environment whichever rows the call holds — and reset[B] marks rows whose environment begins an episode (they plan cold).
        Both are ignored without warm start."""
        if self.task is not None:
            raise ValueError('task= scores the trajectories of ONE plan out of one buffer; generate_actions plans on a batch handle, which the '
                             'task scorer does not serve: use generate_action')
        if self.shift_elites:
            raise ValueError('shift_elites=True carries elites across the plans of ONE environment; generate_actions plans on a batch handle, '
                             'whose rows move between slots: use generate_action, or keep_elites alone')
        if self.replan_every > 1:
            raise ValueError('replan_every = %d keeps ONE sequence between plans; generate_actions plans on a batch handle, for whose rows '
                             'no sequences are kept: use generate_action, or replan_every = 1' % self.replan_every)
        if self.population_decay is not None or self.mean_candidate:
            raise ValueError('population_decay / mean_candidate give every iteration of ONE plan its own launches; generate_actions plans on a '
                             'batch handle, which launches the tiles of one plan for all its rows and serves neither: use generate_action')
        st = np.asarray(states, np.float32)
        if st.ndim != 2:
            raise ValueError('states must be [B, obs_dim]')
        warm = {}                                      # plan_batch's extra arguments with warm start: the rows' slots and call numbers
        if self.warm_start:
            sl = np.arange(st.shape[0], dtype=np.int32) if slots is None else np.asarray(slots, np.int32).reshape(-1)
            if sl.shape != (st.shape[0],):
                raise ValueError('slots must have one entry per row of states')
            pl = self.build_batch(max(st.shape[0], int(sl.max()) + 1))
            if reset is not None:
                for s in sl[np.asarray(reset, bool).reshape(-1)]:
                    pl.reset_carry(int(s))
            warm = dict(slots=sl, calls=np.array(self._next_calls(sl), np.uint64))
        else:
            pl = self.build_batch(st.shape[0])
            warm = dict(calls=pl.take_calls(st.shape[0]))           # the numbers plan_batch would draw itself, kept for SafeCemMpc's recovery
        actions, scores, iters = pl.plan_batch(st, seed=self.seed, **warm)
        self.last_scores, self.last_iterations, self.last_calls = scores, iters, warm['calls']
        self._note_ess(pl, iters)
        if self.plan_readout:
            self.last_plans = [pl.plan_readout(b) for b in range(st.shape[0])]
        return actions

    def do_generate_action(self, state, eps_act=None, eps_model=None, eps_out=None):
        """(action, best_score) like cem_mpc.py:35-68; explicit noise tensors replace TF's stateful RNG."""
        self.build()
        self._stage_clock(self._planner)
        action, score, iters = self._planner.plan(np.asarray(state, np.float32), seed=self.seed, eps_act=eps_act,
                                                  eps_model=eps_model, eps_out=eps_out)
        self.last_iterations = iters
        return action, score
