"""Elite carry-over on the host: planner.keep_elites / inject_elites / score_keys / elite_keep_count on hand-made inputs (tie order, the
two zeros, NaN and the infinities, m = k, the shifted tail), the case table's own claims, and the oracle seeds it lists — for each the
fp32 oracle's replay keeps both cuts (the k-th place of the population, the m-th of the elites) wider than ORACLE_GAP in every iteration."""
import numpy as np
import pytest

from ethz_safe_learning_amd import PlannerConfig, planner
from ethz_safe_learning_amd.planner import elite_keep_count, inject_elites, keep_elites, score_keys
from tests import elite_cases as ec
from tests import select_cases as sc

F, U = np.float32, np.uint32


def _actions(n, h=3, a=2):
    """Row n holds n + (step, dimension) / 1000: a row says which candidate it was."""
    return (np.arange(n, dtype=F)[:, None, None] + (np.arange(h * a, dtype=F).reshape(h, a) / F(1000))).astype(F)


def _rows(E):
    return [int(round(float(r[0, 0]))) for r in E]


def _keep_reference(scores, elite, m):
    """The contract as a Python sort over (key descending, candidate index ascending)."""
    keys = score_keys(np.asarray(scores, F))
    return sorted((int(e) for e in elite), key=lambda e: (-int(keys[e]), e))[:m]


def test_score_keys_order_values_like_the_select():
    v = np.array([np.nan, -np.inf, -3.5, -1e-45, -0.0, 0.0, 1e-45, 2.0, np.inf], F)
    k = score_keys(v)
    assert k[0] == 0 and k[4] == k[5] == 0x80000000
    assert np.all(np.diff(np.delete(k, 4).astype(np.int64)) > 0)                  # strictly ascending once one of the zeros is dropped
    for bits in (0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFC12345):
        assert score_keys(np.array([bits], U).view(F))[0] == 0
    # select_cases.key2f is the inverse wherever a key has one
    keys = np.array([0x007FFFFF, 0x3F7FFFFF, 0x7FFFFFFE, 0x80000000, 0xBF800000, 0xFF800000], U)
    np.testing.assert_array_equal(score_keys(sc.key2f(keys)), keys)


def test_keep_orders_by_score_then_by_lower_index():
    a = _actions(12)
    scores = np.array([0, 5, 1, 5, 9, 5, 2, 9, 0, 0, 5, 1], F)
    elite = np.array([1, 3, 4, 5, 7, 10], np.int32)                               # ascending, as the select stores them
    assert _rows(keep_elites(scores, elite, a, 6)) == [4, 7, 1, 3, 5, 10]
    assert _rows(keep_elites(scores, elite, a, 3)) == [4, 7, 1]                   # the cut inside the run of fives: the lowest index
    assert _rows(keep_elites(scores, elite[::-1].copy(), a, 3)) == [4, 7, 1]      # whatever order the indices come in
    assert keep_elites(scores, elite, a, 0).shape == (0, 3, 2)
    np.testing.assert_array_equal(keep_elites(scores, elite, a, 2).view(U), a[[4, 7]].view(U))      # exact copies
    with pytest.raises(ValueError):
        keep_elites(scores, elite, a, 7)


def test_keep_ties_the_two_zeros_and_puts_nan_below_minus_infinity():
    a = _actions(8)
    scores = np.array([-0.0, 0.0, -1.0, 0.0, -0.0, np.nan, -np.inf, 3.0], F)
    assert _rows(keep_elites(scores, np.arange(8, dtype=np.int32), a, 8)) == [7, 0, 1, 3, 4, 2, 6, 5]
    # value order with +0 above -0 would give 1, 3 before 0, 4: the keys make them one run
    assert _rows(keep_elites(scores, np.array([0, 1, 3, 4], np.int32), a, 2)) == [0, 1]
    for bits in (0x7FC00000, 0xFFC00000, 0x7F800001):                             # every NaN, either sign, sorts last and ties with the others
        s = scores.copy()
        s[[2, 5]] = np.array([bits, 0xFFC12345], U).view(F)
        assert _rows(keep_elites(s, np.arange(8, dtype=np.int32), a, 8))[-3:] == [6, 2, 5]


@pytest.mark.parametrize('m', [1, 3, ec.K])
def test_keep_on_the_adversarial_vectors_is_the_sorted_reference(m):
    a = _actions(ec.N)
    for name, scores in ec.adversarial_scores(ec.N, ec.K, m).items():
        elite = sc.reference_top_k(scores, ec.K).astype(np.int32)
        want = _keep_reference(scores, elite, m)
        assert _rows(keep_elites(scores, elite, a, m)) == want, name
        if name in ('all_equal', 'signed_zeros'):
            assert want == sorted(want) and want == elite[:m].tolist(), name     # all elites tie: the lowest indices, whatever the zero's sign
    adv = ec.adversarial_scores(ec.N, ec.K, m)
    assert np.isnan(adv['nan_elites'][sc.reference_top_k(adv['nan_elites'], ec.K)]).any()            # NaNs do reach the elite set
    assert np.isinf(adv['infinities']).sum() == 2


def test_inject_copies_rows_and_leaves_the_shifted_tail_alone():
    n, h, a_dim = 9, 5, 3
    drawn = _actions(n, h, a_dim)
    E = -_actions(4, h, a_dim) - F(100)
    out = inject_elites(drawn, E, 4, 0)
    np.testing.assert_array_equal(out[:4].view(U), E.view(U))
    np.testing.assert_array_equal(out[4:].view(U), drawn[4:].view(U))
    for s in (1, h - 1):
        out = inject_elites(drawn, E, 3, s)
        np.testing.assert_array_equal(out[:3, :h - s].view(U), E[:3, s:].view(U))                   # moved towards the present
        np.testing.assert_array_equal(out[:3, h - s:].view(U), drawn[:3, h - s:].view(U))           # the freed tail: the sampler's draw
        np.testing.assert_array_equal(out[3:].view(U), drawn[3:].view(U))                           # E[3] is beyond count
    np.testing.assert_array_equal(inject_elites(drawn, E, 0, 1).view(U), drawn.view(U))             # count 0: nothing
    np.testing.assert_array_equal(inject_elites(drawn, E, 4, h).view(U), drawn.view(U))             # everything is tail
    assert inject_elites(drawn, E, 9, 0)[4:].tobytes() == drawn[4:].tobytes()                       # never more rows than the store has
    assert drawn is not inject_elites(drawn, E, 0) and drawn[0, 0, 0] == 0                          # a copy
    with pytest.raises(ValueError):
        inject_elites(drawn, E, 1, h + 1)


def test_keep_count_of_a_fraction():
    assert [elite_keep_count(f, 10) for f in (0.3, 0.05, 1.0, 0.99)] == [3, 1, 10, 9]
    assert elite_keep_count(0.3, 50) == 15 and elite_keep_count(0.3, 1) == 1
    for bad in (0.0, -0.1, 1.5, float('nan')):
        with pytest.raises(ValueError):
            elite_keep_count(bad, 10)


def test_planner_config_fields():
    names = list(PlannerConfig.__dataclass_fields__)
    i = names.index('keep_elites')
    assert names[i:i + 3] == ['keep_elites', 'shift_elites', 'elite_shift'] and names[i - 1] == 'action_noise_param' and names[i + 3] == 'worst_particles'
    pb = ec.problem(ec.BY_NAME['lean_one_quad'])
    from tests import helpers as hp
    _, cfg = hp.configs(pb, **ec.config_kwargs(ec.BY_NAME['lean_one_quad']))
    assert (cfg.keep_elites, cfg.shift_elites, cfg.elite_shift) == (0, False, 1)
    import dataclasses
    on = dataclasses.replace(cfg, keep_elites=3)
    assert planner.config_key(on) != planner.config_key(cfg)
    assert planner.config_key(dataclasses.replace(on, shift_elites=True)) != planner.config_key(on)
    assert bytes(planner.to_c_config(on)) == bytes(planner.to_c_config(cfg))     # not in cem_config_t: set after create


def test_case_table_covers_what_it_claims():
    by = ec.BY_NAME
    assert {c.m for c in ec.CASES} >= {1, 3, ec.K} and {c.H for c in ec.CASES} >= {1, 2, 5}
    assert {c.variant for c in ec.CASES} == {'cem', 'safe', 'cost'}
    assert {c.shift for c in ec.ACROSS_CASES} >= {1} and any(c.shift == c.H - 1 and c.H > 2 for c in ec.ACROSS_CASES)
    assert all(1 <= c.m <= c.k < c.N and (c.E * c.N) % c.E == 0 for c in ec.CASES)
    assert all(1 <= c.shift < c.H for c in ec.ACROSS_CASES) and by['h1'] not in ec.ACROSS_CASES
    assert ec.pad_layout(by['lean_one_quad']) == (4, 0)                          # one quad, aligned
    assert ec.pad_layout(by['two_quads']) == (8, 2)                              # two quads, the actions start at word 2
    assert ec.pad_layout(by['two_blocks']) == (8, 2)
    assert by['two_blocks'].obs + by['two_blocks'].act > 64 and by['wide256'].units == 256 and by['bf16x3'].precision == 'bf16x3'
    assert by['segments'].segments > 1 and by['segments'].N == 40
    assert all(c.variant != 'cost' or not c.oracle_seeds for c in ec.CASES)


@pytest.mark.parametrize('case,seed', ec.ORACLE_CASES, ids=['%s_seed%d' % (c.name, s) for c, s in ec.ORACLE_CASES])
def test_oracle_seeds_keep_both_cuts_clear_of_rounding(case, seed):
    _, score, iters, trace = ec.oracle_plan(case, seed)
    assert iters == ec.I and np.isfinite(score)
    gaps = ec.oracle_gaps(trace, case.k, case.m)
    print('%s seed %d: gaps (k-th place, m-th elite) per iteration %s' % (case.name, seed, gaps))
    assert all(gk > ec.ORACLE_GAP and gm > ec.ORACLE_GAP for gk, gm in gaps), gaps
    # the carry is live in the replay: rows 0 .. m - 1 of iterations >= 1 are the previous store, and some carried row is elite again
    for it in range(1, iters):
        np.testing.assert_array_equal(trace[it]['actions'][:case.m].view(U), trace[it - 1]['store'].view(U))
    assert any((np.asarray(trace[it]['elite']) < case.m).any() for it in range(1, iters))
