// cem_plan_options.h — the options a planner handle launches its plans with, as one value, and the one place that says which
// combinations a handle admits.  Host code only, nothing of HIP: cem_capi.hip's setters are its users, tests/native/option_rules_main.cpp
// runs admit() on its own.
//
// A setter takes `next`, a copy of the handle's PlanOptions with its own change applied, asks admit(facts, next), prepares what it
// needs and commits `next` (cem_capi.hip: commit_launch_change).  cem_planner_comm_init does the same with next.comm = true.  The rules are
// about the COMBINATION, so they hold whichever call comes first ("The option rules").
#pragma once
#include <cstdint>
#include <vector>
#include "../../include/cem_mpc.h"

struct PlanOptions {
    int tail_m = 0;                          // cem_planner_set_particle_objective: 0 = the particle mean, 1 .. P = the mean of the m smallest returns (cem_score.h)
    int cost_m = 0;                          // cem_planner_set_constraint: 0 = CEM_CONSTRAINT_BETA; 1 .. P = CEM_CONSTRAINT_BUDGET on the m largest particle costs (P: their mean)
    int refit_kind = CEM_REFIT_UNIFORM;      // cem_planner_set_refit: CEM_REFIT_SOFTMAX puts cem_constraint_refit_kernel behind the select (cem_refit_weighted.h)
    float refit_tau = 0.f;                   // the temperature as set
    int noise_kind = CEM_NOISE_WHITE;        // cem_planner_set_action_noise: CEM_NOISE_MIXED lets the samplers read the handle's mixed tensor (cem_noise_mix.h)
    cem_elite_carry_t elite{0, 0, 1, 0};     // cem_planner_set_elite_carry, as set; n_keep 0: off (cem_elite_carry.h)
    std::vector<int32_t> pop;                // cem_planner_set_population_schedule: n[it] of every iteration; empty: off (cem_population.h)
    int mean_cand = 0;                       // cem_planner_set_mean_candidate: 1 = the last iteration's last candidate is the clipped mean
    int readout = 0;                         // cem_planner_set_plan_readout: 1 = cem_plan_track_kernel follows every select (cem_plan_readout.h)
    int task = 0;                            // cem_planner_set_task / _set_task_tracking: the kind; CEM_TASK_QUADRATIC puts cem_task_score_kernel behind a MODE 1 rollout
                                             // (cem_task_score.h), CEM_TASK_TRACKING cem_task_reference_kernel (cem_task_reference.h): two kinds of one tile (cem_task_tile.h); admit() treats the two alike
    int zones = 0;                           // cem_planner_set_task_zones: the number of zones on the task in force; not 0: cem_task_zones_kernel takes the task
                                             // kernel's place (cem_task_zones.h); recipe and launch count are the base task plan's
    int outputs = 0;                         // cem_planner_set_task_outputs: the number of linear outputs on the task in force; not 0: cem_task_outputs_kernel takes
                                             // the task's (or the zones') kernel's place (cem_task_outputs.h); recipe and launch count are the base task plan's
    bool comm = false;                       // the handle has a communicator (cem_planner_comm_init; cem_capi.hip: options_of reads it off the handle)
};

// What the rules read off a handle (cem_capi.hip: facts_of)
struct HandleFacts {
    int W = 1, batch = 0, variant = CEM_VARIANT_CEM, N = 0, k = 0, H = 0, A = 0, I = 0, P = 0;
    int select_mode = 1;                     // select_mode_for the handle's own population
    std::vector<int> pop_select_mode;        // ... and for every population of the schedule being admitted
    // capacities of the kernels behind the options (their headers' macros)
    int tail_max_p = 0, budget_max_tail_p = 0, elite_max_k = 0, mix_max_h = 0, readout_max_p = 0, max_cost_kinds = 0;
    long long budget_total_limit = 0;                  // H * m * kinds of a budget plan stays below it (cem_capi.hip: kBudgetTotalLimit)
    size_t refit_lds_bytes = 0, refit_lds_limit = 0;   // the weighted refit's dynamic LDS at this (k, H A) and what the device grants
    // the launchers of the optional translation units that are linked in
    bool can_mix = false, can_carry = false, can_mean = false, can_track = false, can_task = false, can_zones = false, can_outputs = false;
};

// which call asks: only the inherited asymmetry below reads it
enum PlanChange { PLAN_CHANGE_OTHER = 0, PLAN_CHANGE_REFIT = 1 };

// CEM_OK or CEM_ERR_UNSUPPORTED.  Each rule once; switching an option off never makes an admitted combination a refused one.
inline int admit(const HandleFacts &f, const PlanOptions &o, PlanChange change = PLAN_CHANGE_OTHER)
{
    const bool tail = o.tail_m != 0, budget = o.cost_m != 0, softmax = o.refit_kind == CEM_REFIT_SOFTMAX, mixed = o.noise_kind == CEM_NOISE_MIXED;
    const bool carry = o.elite.n_keep != 0, sched = !o.pop.empty(), mean = o.mean_cand != 0, track = o.readout != 0;
    // ONE RANK.  Every kernel behind these options is rank-local (one rank's key, one rank's select, a candidate's whole column of
    // returns); no sharded run of any of them has been made, so none is offered
    if (f.W > 1 && (tail || budget || softmax || mixed || carry || sched || mean || track)) return CEM_ERR_UNSUPPORTED;
    // NO COMMUNICATOR, for the same reason — the two objectives excepted, which a world-1 communicator leaves as they are
    if (o.comm && (mixed || carry || sched || mean || track)) return CEM_ERR_UNSUPPORTED;
    // INHERITED ASYMMETRY (an open question for the maintainer, not a rule): cem_planner_set_refit refuses a handle that has a
    // communicator, cem_planner_comm_init has never refused a handle with the softmax refit — the answer depends on the order of the
    // two calls, as it did before the rules were gathered here.  Settling it means moving `softmax` into the rule above.
    if (o.comm && softmax && change == PLAN_CHANGE_REFIT) return CEM_ERR_UNSUPPORTED;
    // THE ONE-WORKGROUP SELECT.  The multi-workgroup forms keep their own moment kernels, which the refit kernel does not replace, and
    // the keep / tracker read the one-workgroup select's elite list; a schedule's populations are ranked by that kernel too
    if (softmax || carry || sched || mean || track) {
        if (f.select_mode != 1) return CEM_ERR_UNSUPPORTED;
        for (int m : f.pop_select_mode) if (m != 1) return CEM_ERR_UNSUPPORTED;
    }
    // A SINGLE-STATE HANDLE.  A batch handle's launch carries every problem's tiles of ONE plan, and its rows move between slots
    // (cem_planner_set_carry_slots)
    if (f.batch && (sched || mean || (carry && o.elite.across_plans))) return CEM_ERR_UNSUPPORTED;
    // THE VARIANT.  CEM_VARIANT_COST has no returns to take a tail of; the budget reads the SAFE rollout's masked cost bytes
    if (tail && f.variant == CEM_VARIANT_COST) return CEM_ERR_UNSUPPORTED;
    if (budget && f.variant != CEM_VARIANT_SAFE) return CEM_ERR_UNSUPPORTED;
    // ONE m.  A lower tail of the returns within a cost budget is not offered (the score kernels share ReduceParams::m)
    if (tail && budget) return CEM_ERR_UNSUPPORTED;
    // CAPACITIES of the kernels, and THE KERNELS THEMSELVES (a library built from cem_capi.hip alone has none of the four)
    if (tail && f.P > f.tail_max_p) return CEM_ERR_UNSUPPORTED;
    if (budget && ((o.cost_m < f.P && f.P > f.budget_max_tail_p) || (long long)f.H * o.cost_m * f.max_cost_kinds >= f.budget_total_limit)) return CEM_ERR_UNSUPPORTED;
    if (softmax && f.refit_lds_bytes > f.refit_lds_limit) return CEM_ERR_UNSUPPORTED;
    if (mixed && (f.H > f.mix_max_h || !f.can_mix)) return CEM_ERR_UNSUPPORTED;
    if (carry && (f.k > f.elite_max_k || !f.can_carry)) return CEM_ERR_UNSUPPORTED;
    if (mean && !f.can_mean) return CEM_ERR_UNSUPPORTED;
    if (track && (f.P > f.readout_max_p || !f.can_track)) return CEM_ERR_UNSUPPORTED;
    // THE TASK SCORER reads every row's whole trajectory out of ONE buffer of a single-state, single-rank handle (cem_task_score.h): no
    // shard, no communicator, no batch handle, and the kernel itself
    if (o.task != 0 && (f.W > 1 || o.comm || f.batch || !f.can_task)) return CEM_ERR_UNSUPPORTED;
    // ZONES need their kernel, which stands in for the task's own (cem_task_zones.h); that they sit on a task is the setters' business:
    // cem_planner_set_task_zones wants one in force, cem_planner_set_task clears them
    if (o.zones != 0 && !f.can_zones) return CEM_ERR_UNSUPPORTED;
    if (o.outputs != 0 && !f.can_outputs) return CEM_ERR_UNSUPPORTED;   // OUTPUTS likewise (cem_task_outputs.h)
    // THE INJECT'S ROWS are candidates of every iteration, and none of them is the mean candidate's (the last iteration's last row)
    if (carry) {
        for (int32_t n : o.pop) if (n <= o.elite.n_keep) return CEM_ERR_UNSUPPORTED;
        const int n_last = sched ? o.pop.back() : f.N;
        if (mean && o.elite.n_keep >= n_last - 1) return CEM_ERR_UNSUPPORTED;
    }
    return CEM_OK;
}
