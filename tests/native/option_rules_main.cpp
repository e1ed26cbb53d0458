// option_rules_main.cpp — the option rules of a planner handle (csrc/cem_plan_options.h: admit) on their own: no HIP, no library, no GPU.
// tests/test_option_rules_cpu.py builds this with the host compiler and -fsanitize=address,undefined and runs it.
//
// Over a small lattice — the handle kinds of tests/golden/option_statuses.json as HandleFacts, every on / off combination of the
// options with that file's parameter values — it asserts:
//   (a) switching an option off never turns an admitted combination into a refused one (a handle can always be reset);
//   (b) apart from the one named exception (softmax refit x communicator), reaching a combination does not depend on the order of the
//       two calls: if A then B is admitted, so is B then A;
//   (c) a hand-written list of cases, at least one per rule of DESIGN.md's table, gets the stated answer.
#include "../../ethz_safe_learning_amd/csrc/cem_plan_options.h"

#include <cstdio>
#include <functional>
#include <string>

namespace {

const int N = 128, H = 8, P = 5, K = 12, I = 3;
int g_failed = 0;
void expect(bool ok, const std::string &what) { if (!ok) { std::fprintf(stderr, "FAILED: %s\n", what.c_str()); ++g_failed; } }

struct Kind { const char *name; HandleFacts f; int mode; };
HandleFacts facts(int variant, int mode, int W, int batch)
{
    HandleFacts f;
    f.W = W; f.batch = batch; f.variant = variant; f.N = N; f.k = K; f.H = H; f.A = 2; f.I = I; f.P = P;
    f.select_mode = mode;
    // (the shipped kernels' capacities: all far from the smoke shape)
    f.tail_max_p = 64; f.budget_max_tail_p = 64; f.elite_max_k = 1024; f.mix_max_h = 64; f.readout_max_p = 64; f.max_cost_kinds = 4; f.budget_total_limit = 1ll << 23;
    f.refit_lds_bytes = 4096; f.refit_lds_limit = 64 * 1024;
    f.can_mix = f.can_carry = f.can_mean = f.can_track = true;
    return f;
}
const Kind kKinds[] = {
    {"cem", facts(CEM_VARIANT_CEM, 1, 1, 0), 1},         {"safe", facts(CEM_VARIANT_SAFE, 1, 1, 0), 1},
    {"cost", facts(CEM_VARIANT_COST, 1, 1, 0), 1},       {"select2", facts(CEM_VARIANT_CEM, 2, 1, 0), 2},
    {"select3", facts(CEM_VARIANT_CEM, 3, 1, 0), 3},     {"world2", facts(CEM_VARIANT_CEM, 1, 2, 0), 1},
    {"batch2", facts(CEM_VARIANT_CEM, 1, 1, 2), 1},
};

// One option = one setter: its values (0 = off), and how a value is written into a PlanOptions
struct Option { const char *name; int n_values; PlanChange change; std::function<void(PlanOptions &, int)> set; std::function<int(const PlanOptions &)> get; };
int elite_value(const PlanOptions &o) { return o.elite.n_keep == 0 ? 0 : o.elite.n_keep == 12 ? 3 : o.elite.across_plans ? 2 : 1; }
const Option kOptions[] = {
    {"tail", 2, PLAN_CHANGE_OTHER, [](PlanOptions &o, int v) { o.tail_m = v ? 2 : 0; }, [](const PlanOptions &o) { return o.tail_m ? 1 : 0; }},
    {"budget", 2, PLAN_CHANGE_OTHER, [](PlanOptions &o, int v) { o.cost_m = v ? 2 : 0; }, [](const PlanOptions &o) { return o.cost_m ? 1 : 0; }},
    {"softmax", 2, PLAN_CHANGE_REFIT, [](PlanOptions &o, int v) { o.refit_kind = v ? CEM_REFIT_SOFTMAX : CEM_REFIT_UNIFORM; o.refit_tau = v ? 0.5f : 0.f; },
     [](const PlanOptions &o) { return o.refit_kind == CEM_REFIT_SOFTMAX ? 1 : 0; }},
    {"mixed", 2, PLAN_CHANGE_OTHER, [](PlanOptions &o, int v) { o.noise_kind = v ? CEM_NOISE_MIXED : CEM_NOISE_WHITE; },
     [](const PlanOptions &o) { return o.noise_kind == CEM_NOISE_MIXED ? 1 : 0; }},
    {"elite", 4, PLAN_CHANGE_OTHER, [](PlanOptions &o, int v) { o.elite = cem_elite_carry_t{v == 3 ? 12 : v ? 1 : 0, v == 2, 1, 0}; }, elite_value},
    {"schedule", 3, PLAN_CHANGE_OTHER, [](PlanOptions &o, int v) { o.pop.clear(); if (v) o.pop = {128, 64, v == 1 ? 32 : 13}; },
     [](const PlanOptions &o) { return o.pop.empty() ? 0 : o.pop.back() == 32 ? 1 : 2; }},
    {"mean", 2, PLAN_CHANGE_OTHER, [](PlanOptions &o, int v) { o.mean_cand = v; }, [](const PlanOptions &o) { return o.mean_cand; }},
    {"readout", 2, PLAN_CHANGE_OTHER, [](PlanOptions &o, int v) { o.readout = v; }, [](const PlanOptions &o) { return o.readout; }},
    {"comm", 2, PLAN_CHANGE_OTHER, [](PlanOptions &o, int v) { o.comm = v != 0; }, [](const PlanOptions &o) { return o.comm ? 1 : 0; }},
};
const int kNumOptions = (int)(sizeof kOptions / sizeof kOptions[0]);

// what a setter of the library asks: the facts with the select modes of the schedule being admitted, then admit
bool admitted(const Kind &k, const PlanOptions &o, PlanChange change = PLAN_CHANGE_OTHER)
{
    HandleFacts f = k.f;
    f.pop_select_mode.assign(o.pop.size(), k.mode);
    return admit(f, o, change) == CEM_OK;
}
std::string describe(const Kind &k, const PlanOptions &o)
{
    std::string s = k.name;
    for (const Option &op : kOptions) if (op.get(o)) s += std::string(" ") + op.name + "=" + std::to_string(op.get(o));
    return s;
}
void for_every_combination(const std::function<void(const PlanOptions &)> &fn)
{
    int total = 1;
    for (const Option &op : kOptions) total *= op.n_values;
    for (int c = 0; c < total; ++c) {
        PlanOptions o;
        int rest = c;
        for (const Option &op : kOptions) { op.set(o, rest % op.n_values); rest /= op.n_values; }
        fn(o);
    }
}

void check_lattice(const Kind &k, long *n_admitted, long *n_exception)
{
    for_every_combination([&](const PlanOptions &o) {
        if (!admitted(k, o)) return;
        ++*n_admitted;
        // (a) every option of an admitted combination can be switched off, by its own setter
        for (const Option &op : kOptions) {
            if (!op.get(o)) continue;
            PlanOptions off = o; op.set(off, 0);
            expect(admitted(k, off, op.change), "(a) " + describe(k, o) + ": switching " + op.name + " off is refused");
        }
        // (b) from here, A then B is admitted exactly when B then A is
        for (int a = 0; a < kNumOptions; ++a) for (int b = a + 1; b < kNumOptions; ++b) {
            const Option &A = kOptions[a], &B = kOptions[b];
            if (A.get(o) || B.get(o)) continue;
            for (int va = 1; va < A.n_values; ++va) for (int vb = 1; vb < B.n_values; ++vb) {
                PlanOptions oa = o, ob = o; A.set(oa, va); B.set(ob, vb);
                PlanOptions oab = oa; B.set(oab, vb);
                const bool ab = admitted(k, oa, A.change) && admitted(k, oab, B.change);
                const bool ba = admitted(k, ob, B.change) && admitted(k, oab, A.change);
                if (std::string(A.name) == "softmax" && std::string(B.name) == "comm") {
                    // THE NAMED EXCEPTION (cem_plan_options.h, "inherited asymmetry"): the refit's setter refuses a communicator, comm_init
                    // does not refuse the refit
                    expect(!ba, "(b) " + describe(k, o) + ": comm then softmax is admitted");
                    if (ab) ++*n_exception;
                } else
                    expect(ab == ba, "(b) " + describe(k, o) + ": " + A.name + " / " + B.name + " depends on the order");
            }
        }
    });
}

// (c) one rule at a time
struct Case { const char *rule; const char *kind; std::function<void(PlanOptions &)> set; bool want; std::function<void(HandleFacts &)> facts; };
void check_cases()
{
    auto on = [](const char *name, int v = 1) { return [=](PlanOptions &o) { for (const Option &op : kOptions) if (std::string(op.name) == name) op.set(o, v); }; };
    auto both = [](std::function<void(PlanOptions &)> x, std::function<void(PlanOptions &)> y) { return [=](PlanOptions &o) { x(o); y(o); }; };
    const Case cases[] = {
        {"nothing on", "world2", [](PlanOptions &) {}, true, nullptr},
        {"one rank", "world2", on("tail"), false, nullptr},
        {"one rank", "world2", on("readout"), false, nullptr},
        {"one rank: a world-2 handle takes its communicator", "world2", on("comm"), true, nullptr},
        {"no communicator", "cem", both(on("comm"), on("mixed")), false, nullptr},
        {"no communicator", "cem", both(on("comm"), on("elite")), false, nullptr},
        {"no communicator: the objectives keep a world-1 communicator", "safe", both(on("comm"), on("budget")), true, nullptr},
        {"no communicator: the objectives keep a world-1 communicator", "cem", both(on("comm"), on("tail")), true, nullptr},
        {"one-workgroup select", "select2", on("softmax"), false, nullptr},
        {"one-workgroup select", "select3", on("schedule"), false, nullptr},
        {"one-workgroup select: the objectives and the noise do not ask", "select2", both(on("tail"), on("mixed")), true, nullptr},
        {"single-state handle", "batch2", on("schedule"), false, nullptr},
        {"single-state handle", "batch2", on("mean"), false, nullptr},
        {"single-state handle", "batch2", on("elite", 2), false, nullptr},
        {"single-state handle: n_keep alone is served", "batch2", on("elite", 1), true, nullptr},
        {"variant", "cost", on("tail"), false, nullptr},
        {"variant", "cem", on("budget"), false, nullptr},
        {"variant", "safe", on("budget"), true, nullptr},
        {"one m", "safe", both(on("tail"), on("budget")), false, nullptr},
        {"capacity: tail", "cem", on("tail"), false, [](HandleFacts &f) { f.tail_max_p = P - 1; }},
        {"capacity: budget tail", "safe", on("budget"), false, [](HandleFacts &f) { f.budget_max_tail_p = P - 1; }},
        {"capacity: budget total", "safe", on("budget"), false, [](HandleFacts &f) { f.budget_total_limit = (long long)H * 2 * f.max_cost_kinds; }},
        {"capacity: refit LDS", "cem", on("softmax"), false, [](HandleFacts &f) { f.refit_lds_limit = f.refit_lds_bytes - 1; }},
        {"capacity: mixing horizon", "cem", on("mixed"), false, [](HandleFacts &f) { f.mix_max_h = H - 1; }},
        {"capacity: elites", "cem", on("elite"), false, [](HandleFacts &f) { f.elite_max_k = K - 1; }},
        {"capacity: read-out particles", "cem", on("readout"), false, [](HandleFacts &f) { f.readout_max_p = P - 1; }},
        {"kernel present", "cem", on("mixed"), false, [](HandleFacts &f) { f.can_mix = false; }},
        {"kernel present", "cem", on("elite"), false, [](HandleFacts &f) { f.can_carry = false; }},
        {"kernel present", "cem", on("mean"), false, [](HandleFacts &f) { f.can_mean = false; }},
        {"kernel present", "cem", on("readout"), false, [](HandleFacts &f) { f.can_track = false; }},
        {"inject's rows", "cem", both(on("elite", 3), on("schedule", 2)), true, nullptr},              // n_keep 12 with [128, 64, 13]
        {"inject's rows", "cem", both(both(on("elite", 3), on("schedule", 2)), on("mean")), false, nullptr},     // ... and the mean candidate
        {"inject's rows", "cem", both(both(on("elite", 3), on("schedule", 1)), on("mean")), true, nullptr},      // [128, 64, 32]: room for both
        {"inject's rows", "cem", both(on("elite", 3), [](PlanOptions &o) { o.pop = {128, 64, 12}; }), false, nullptr},   // a population of n_keep rows
    };
    for (const Case &c : cases) {
        const Kind *k = nullptr;
        for (const Kind &kk : kKinds) if (std::string(kk.name) == c.kind) k = &kk;
        Kind kind = *k;
        if (c.facts) c.facts(kind.f);
        PlanOptions o; c.set(o);
        expect(admitted(kind, o) == c.want, std::string("(c) ") + c.rule + ": " + describe(kind, o) + " should be " + (c.want ? "admitted" : "refused"));
    }
    // the named exception, both ways round
    PlanOptions o; o.comm = true; o.refit_kind = CEM_REFIT_SOFTMAX; o.refit_tau = 0.5f;
    expect(!admitted(kKinds[0], o, PLAN_CHANGE_REFIT), "(c) inherited asymmetry: set_refit on a handle with a communicator should be refused");
    expect(admitted(kKinds[0], o, PLAN_CHANGE_OTHER), "(c) inherited asymmetry: comm_init on a handle with the softmax refit should be admitted");
}

}  // namespace

int main()
{
    long n_admitted = 0, n_exception = 0;
    for (const Kind &k : kKinds) check_lattice(k, &n_admitted, &n_exception);
    expect(n_admitted > 0 && n_exception > 0, "the lattice holds admitted combinations and the named exception");
    check_cases();
    std::printf("%ld admitted combinations on %d handle kinds, the named exception met %ld times, %d failed\n",
                n_admitted, (int)(sizeof kKinds / sizeof kKinds[0]), n_exception, g_failed);
    return g_failed ? 1 : 0;
}
