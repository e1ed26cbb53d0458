"""The committed seed tables of tests/bf16_fuzz_cases.py, screened without a device: every seed tests/test_gpu_bf16_fuzz.py runs is
admitted by the conditions stated there — the configuration accepted, few candidates on a threshold, the fp32-accumulating stand-in
within HALF the bar under all 24 chunk orders, every mutant caught — and the tables cover what the kernel has a path for."""
import numpy as np
import pytest

from tests import bf16_cases as bc
from tests import bf16_fuzz_cases as fz


def test_the_tables_have_their_sizes_and_no_dropped_seed():
    assert len(set(fz.SCORE_SEEDS)) == len(fz.SCORE_SEEDS) == 32
    assert len(set(fz.UNFOLD_SEEDS)) == len(fz.UNFOLD_SEEDS) == 16
    assert len(set(fz.CUT_SEEDS)) == len(fz.CUT_SEEDS) == 12
    tables = dict(score=fz.SCORE_SEEDS, unfold=fz.UNFOLD_SEEDS, cut=fz.CUT_SEEDS)
    assert all(seed not in tables[table] for table, seed in fz.DROPPED)
    assert len(bc.ORDERS) == 24 and len(set(map(tuple, bc.ORDERS))) == 24
    assert [list(p) for p in bc.ORDERS[:3]] == [[1, 3, 0, 2], [3, 2, 1, 0], [2, 0, 3, 1]]        # the fixed cases' orders stay orders 0 - 2


def test_the_dropped_seed_is_reproduced_by_a_cpu_summation_order():
    """A seed leaves a table only if a CPU summation order reproduces what the device showed (bf16_fuzz_cases.DROPPED): unfold seed 12
    passes under every chunk order at half the bar, and with a float32 rounding after every product misses the RMS bar on mu at the
    step the device missed it at, by the device's figures."""
    import functools
    assert set(fz.DROPPED) == {('unfold', 12)}
    u = fz.unfold_case(12)
    for order in range(len(bc.ORDERS)):
        fz.check_unfold(fz.unfold_under(u, functools.partial(bc.emu32, order=order)), u, 'order %d' % order, bc.RATIO / 2)
    got = fz.unfold_under(u, functools.partial(bc.emu32, group=1, descending=True))
    K = [bc.rms(got[1][:, t] - u['emu'][1][:, t]) for t in range(6)]
    assert max(K[:3] + K[4:5]) < 1e-9 and 2.0e-6 < K[3] < 2.3e-6 and 1.2e-6 < K[5] < 1.4e-6, K        # the device: 2.16e-6 at step 3, 1.32e-6 at step 5
    with pytest.raises(AssertionError, match='mu step 3'):
        fz.check_unfold(got, u, 'group 1')


@pytest.mark.parametrize('seed', fz.SCORE_SEEDS)
def test_score_seed_is_admitted(seed):
    r = fz.screen_score(seed)
    c = r['c']
    assert c['N'] >= 24 and c['N'] <= 256 and c['H'] <= 12 and c['units'] <= 128
    print('score seed %d: largest stand-in ratios over 24 orders RMS %.4f median %.4f 90th percentile %.4f; mutants caught by %s' % (
        seed, *r['worst'], {k: '+'.join(v) for k, v in r['caught'].items()}))


@pytest.mark.parametrize('seed', fz.UNFOLD_SEEDS)
def test_unfold_seed_is_admitted(seed):
    r = fz.screen_unfold(seed)
    c = r['c']
    assert c['B'] % c['E'] == 0 and c['B'] <= 40 * c['E'] and c['H'] <= 8
    print('unfold seed %d: largest stand-in ratios over 24 orders trajectory %.4f mu %.4f sd %.4f; mutants caught by %s' % (seed, *r['worst'], r['caught']))


@pytest.mark.parametrize('seed', fz.CUT_SEEDS)
def test_cut_seed_is_admitted(seed):
    c, _, cfgs = fz.cut_configs(seed)
    assert c['W'] in (2, 3, 4) and c['rc_full'] != c['rc_shard'] and c['N'] <= 256 and len(cfgs) == 1 + c['W']
    for key, pcfg in cfgs.items():
        st, rc, cnt = fz.tiles_of(pcfg)
        assert st == 0 and cnt.sum() == c['P'] * c['N'] // key[0], (seed, key, st)
        want = c['rc_full'] if key[0] == 1 else c['rc_shard']
        assert rc == want or want == 0, (seed, key, rc)


def test_the_tables_cover_the_kernels_paths():
    """Every depth, every tile size and the automatic one, padded and minimal widths, the input widths on either side of the layer-0
    chunk counts (obs + act <= 32: one chunk of two, = 64, = 65: NFW switches, >= 97: four chunks), members that split a particle,
    one member, sampling off, scaling off, an unbounded box, both objectives — among the score seeds; the unfold seeds cover the
    depths, widths and input widths again, and the cutting seeds every world size and both objectives.
    One-row tiles (td.cnt = 1: every lane's slot clamped to row 0): build_plan_tiles splits a member's run of rows EVENLY, so a
    single rank's plan has none even where P N / E = 1 (mod 16) (several score seeds have that, and tiles of unequal length); they
    arise in cem_unfold_sequences, whose tiles are 16 rows and a tail (an unfold seed with B / E = 1 (mod 16)), and in a sharded plan
    where a rank boundary lies one row past a member boundary (two cutting seeds)."""
    S = [fz.score_params(s) for s in fz.SCORE_SEEDS]
    facts = [fz.tiles_of(fz.score_configs(s)[3]) for s in fz.SCORE_SEEDS]
    assert {c['L'] for c in S} == {1, 2, 3, 4, 5}
    assert {c['rc'] for c in S} == {0, 1, 2, 3, 4} and {rc for _, rc, _ in facts} == {1, 2, 3, 4}
    assert any(c['units'] % 16 for c in S) and any(c['units'] == 16 for c in S) and any(c['units'] == 128 for c in S)
    D = [c['O'] + c['A'] for c in S]
    assert any(d <= 32 for d in D) and 64 in D and 65 in D and any(d >= 97 for d in D)
    assert sum((c['P'] * c['N'] // c['E']) % 16 == 1 for c in S) >= 3, 'several populations with P N / E = 1 (mod 16)'
    assert any(cnt.min() <= 8 for _, _, cnt in facts) and any(len(set(cnt.tolist())) > 1 for _, _, cnt in facts), 'short tiles, and tiles of unequal length'
    assert any(c['P'] % c['E'] for c in S) and any(c['E'] == 1 for c in S)
    assert any(not c['sampling'] for c in S) and any(not c['scale'] for c in S)
    assert any(c['box'] == 'unbounded' for c in S) and any(c['box'] == 'mixed' for c in S) and any(c['box'] == 'asym' for c in S)
    assert {c['variant'] for c in S} == {'cem', 'safe'}
    U = [fz.unfold_params(s) for s in fz.UNFOLD_SEEDS]
    assert {c['L'] for c in U} == {1, 2, 3, 4, 5} and any(c['units'] % 16 for c in U)
    D = [c['O'] + c['A'] for c in U]
    assert any(d <= 32 for d in D) and any(33 <= d <= 64 for d in D) and any(65 <= d <= 96 for d in D) and any(d >= 97 for d in D)
    assert any(not c['sampling'] for c in U) and any(not c['scale'] for c in U) and any(c['E'] == 1 for c in U)
    assert any((c['B'] // c['E']) % 16 == 1 for c in U), 'a one-row tail tile'
    X = [fz.cut_params(s) for s in fz.CUT_SEEDS]
    assert {c['W'] for c in X} == {2, 3, 4} and {c['variant'] for c in X} == {'cem', 'safe'}
    assert any(c['P'] % c['E'] for c in X) and any(c['O'] + c['A'] > 64 for c in X) and any(c['box'] == 'unbounded' for c in X)
    assert {c['rc_full'] for c in X} | {c['rc_shard'] for c in X} == {0, 1, 2, 3, 4}
    shard_tiles = [fz.tiles_of(pcfg)[2] for s in fz.CUT_SEEDS for key, pcfg in fz.cut_configs(s)[2].items() if key[0] > 1]
    assert sum(bool((cnt == 1).any()) for cnt in shard_tiles) >= 2, 'planning tiles of one row (a rank boundary one row past a member boundary)'
