"""The vectors of tests/select_cases.py take the paths they claim — checked on a NumPy model of the one-workgroup cached select's
ROUTING only (which bucket, how many keys, which ending; no ranking, no moments) — and every tie case tells the tie rules apart.
No GPU."""
import numpy as np
import pytest

from oracle import cem_oracle as o
from tests import select_cases as sc

U = np.uint32

# ---- the kernel's constants, restated once (csrc/cem_device.h, cem_select_kernel and cem_f2key; csrc/cem_capi.hip, resolve_select_mode)
BUCKETS = 2048                          # "h2k[2048] bucket counts"; cem_ms_find<false>(h2k, 2048, ...)
TOP_SHIFT = 21                          # "sh = window ? max(0, 21 - clz(window)) : 0": window >> sh < 2048
LEVEL_BITS = 11                         # "sh = sh > 11 ? sh - 11 : 0": a bucket is split 11 bits finer
LEVELS = 4                              # "for (int level = 0; level < 4; ++level)"
DIRECT_MAX = {False: 256, True: 32}     # "if (m <= (CROWDED ? 32u : 256u))": m threads rank the bucket directly
QUARTERS_MAX = 256                      # "if (CROWDED && m <= 256u)": the collected list ranked by quarters, span = (m + 3) >> 2
LDS_LIMIT = 140 * 1024                  # resolve_select_mode: elite list + two [HA] arrays + CEM_SEL_KWORDS(N) key words must fit
HA = 6                                  # H = 3, A = 2 of the GPU harness
NAN_KEY = 0                             # "NaN sorts lowest"


def f2key(x, zeros_tie=True):
    """cem_f2key: NaN -> 0; a negative float's bits inverted, any other float's bits with the sign set; -0.0 takes +0.0's key
    (zeros_tie False: the transform before that, which ranks +0.0 strictly above -0.0)."""
    u = sc.f2bits(x).copy()
    nan = (u & U(0x7FFFFFFF)) > U(0x7F800000)
    if zeros_tie:
        u[u == U(0x80000000)] = U(0)
    key = np.where(u & U(0x80000000), ~u, u | U(0x80000000)).astype(U)
    key[nan] = NAN_KEY
    return key


def cached(N, k):
    """resolve_select_mode's `cache`: CEM_SEL_KWORDS(N) = N + N / 32 + 1 words next to the elite list and the two [HA] arrays."""
    base = ((k + 3) & ~3) * 4 + 2 * HA * 4
    return k <= 24576 and base + (N + (N >> 5) + 1) * 4 <= LDS_LIMIT


def route(keys, k, crowded):
    """(level, m, ending) of cem_select_kernel<true, crowded> on these keys, and the key T and the ties to take it arrives at when the
    ending is 'one_key' (else None): base / window / sh, the bucket counts, cem_ms_find's rule, the thresholds."""
    keys = keys.astype(np.int64)
    base, window = int(keys.min()), int(keys.max() - keys.min())
    sh = max(0, window.bit_length() - (32 - TOP_SHIFT)) if window else 0     # 21 - clz(window) on 32 bits
    need = k
    for level in range(LEVELS):
        off = keys - base
        inside = (off >= 0) & (off <= window)
        counts = np.bincount(off[inside] >> sh, minlength=BUCKETS)
        assert counts.size == BUCKETS                                        # window >> sh < 2048
        ge = np.cumsum(counts[::-1])[::-1]                                   # ge[b] = keys in buckets >= b
        bucket = int(np.nonzero(ge >= need)[0].max())                        # ge[bucket] >= need > ge[bucket + 1]
        need1 = need - (int(ge[bucket + 1]) if bucket + 1 < BUCKETS else 0)
        m = int(counts[bucket])
        assert 1 <= need1 <= m
        if sh == 0:
            return (level, m, 'one_key'), (base + bucket, need1)
        if m <= DIRECT_MAX[crowded]:
            return (level, m, 'direct'), None
        if crowded and m <= QUARTERS_MAX:
            return (level, m, 'quarters'), None
        base, window, need = base + (bucket << sh), (1 << sh) - 1, need1
        sh = sh - LEVEL_BITS if sh > LEVEL_BITS else 0
    raise AssertionError('the bucket select never leaves its loop unsolved: sh reaches 0 by level 2')


def kth_bucket(case):
    """(members in candidate order, their keys, need1) of the k-th key's level-0 bucket."""
    keys = f2key(case.scores).astype(np.int64)
    base, window = int(keys.min()), int(keys.max() - keys.min())
    sh = max(0, window.bit_length() - (32 - TOP_SHIFT))
    b = (keys - base) >> sh
    counts = np.bincount(b, minlength=BUCKETS)
    ge = np.cumsum(counts[::-1])[::-1]
    bucket = int(np.nonzero(ge >= case.k)[0].max())
    members = np.nonzero(b == bucket)[0]
    return members, keys[members], case.k - int(ge[bucket + 1])


CACHED = [c for c in sc.CASES if c.claim[False][2] != 'radix']
UNCACHED = [c for c in sc.CASES if c.claim[False][2] == 'radix']


def test_routing_table():
    """The table the GPU test's cases are read from (pytest -s prints it)."""
    for c in sc.CASES:
        if c in UNCACHED:
            print('%-24s N %5d k %5d  uncached: byte-wide radix passes' % (c.name, c.N, c.k))
        else:
            r = [route(f2key(c.scores), c.k, cr)[0] for cr in (False, True)]
            print('%-24s N %5d k %5d  plain: level %d m %4d %-8s  CROWDED: level %d m %4d %s' % ((c.name, c.N, c.k) + r[0] + r[1]))


@pytest.mark.parametrize('crowded', [False, True])
@pytest.mark.parametrize('case', sc.CASES, ids=lambda c: c.name)
def test_case_takes_the_path_it_claims(case, crowded):
    assert case.scores.dtype == np.float32 and case.scores.shape == (case.N,)
    if case in UNCACHED:
        assert not cached(case.N, case.k) and case.claim[crowded] == (None, None, 'radix')
        return
    assert cached(case.N, case.k)
    got, one_key = route(f2key(case.scores), case.k, crowded)
    assert got == case.claim[crowded], (case.name, crowded, got)
    if one_key:                                                   # 'one_key': only ties remain, and fewer than all unless k covers them
        T, need = one_key
        assert (f2key(case.scores) == T).sum() == got[1] and 1 <= need <= got[1]


def test_every_ending_is_reached_at_every_level_it_can_occur():
    """sh is at most 21 at level 0, at most 10 at level 1 and 0 at level 2: a direct or quarter rank can end levels 0 and 1, a
    one-key bucket any of the three; level 3 is never entered."""
    for crowded in (False, True):
        seen = {route(f2key(c.scores), c.k, crowded)[0][::2] for c in CACHED}
        want = {(0, 'direct'), (1, 'direct'), (0, 'one_key'), (1, 'one_key'), (2, 'one_key')}
        if crowded:
            want |= {(0, 'quarters'), (1, 'quarters')}
        assert seen == want, (crowded, sorted(seen ^ want))


def test_sizes_keep_the_clamps_live():
    for c in sc.CASES:
        if c.name == 'signed_zero_pair' or c in UNCACHED:
            assert c.N in (64, 40000)
        else:
            assert c.N % 32 and c.N > 1024, c.name                # (hence no multiple of 64 or 1024 either) and more than one 1024-thread stride


@pytest.mark.parametrize('case', [c for c in sc.CASES if not c.nan], ids=lambda c: c.name)
def test_reference_is_the_oracles_top_k(case):
    np.testing.assert_array_equal(sc.reference_top_k(case.scores, case.k), o.top_k(case.scores, case.k))
    assert sc.best_of(case.scores, o.top_k(case.scores, case.k)) == o.best_of_elite(case.scores, o.top_k(case.scores, case.k))


@pytest.mark.parametrize('case', [c for c in sc.CASES if c.tie], ids=lambda c: c.name)
def test_tie_case_discriminates(case):
    ref = sc.reference_top_k(case.scores, case.k)
    assert not np.array_equal(ref, sc.top_k_highest_index_first(case.scores, case.k)), 'the cut is not inside a run of equal values'
    if case.signed_zero:
        keys = f2key(case.scores, zeros_tie=False).astype(np.int64)
        by_key = np.sort(np.lexsort((np.arange(case.N), -keys))[:case.k])
        assert not np.array_equal(ref, by_key), 'value order and key order (+0 above -0) agree: the case proves nothing'


def test_tie_flags_are_honest():
    """A case not flagged `tie` really has no tie at its cut (its k-th and (k+1)-th values differ, or k = N)."""
    for c in sc.CASES:
        if not c.tie:
            assert np.array_equal(sc.reference_top_k(c.scores, c.k), sc.top_k_highest_index_first(c.scores, c.k)), c.name


@pytest.mark.parametrize('name', ['mid_m33_need1', 'mid_m255', 'mid_m256', 'mid_m101', 'mid_m64_need_m'])
def test_quarter_ranked_buckets(name):
    """The bucket the CROWDED kernel ranks by quarters: its population, a run of at least three copies of the k-th key whose places in
    the list — taken in candidate order, the order the waves collect it in when they arrive in turn — fall into different quarters."""
    case = sc.BY_NAME[name]
    members, keys, need1 = kth_bucket(case)
    m = members.size
    assert case.claim[True] == (0, m, 'quarters') and members[-1] == case.N - 1 and members[-1] >= 1024
    order = np.lexsort((members, -keys))
    T = keys[order[need1 - 1]]
    places = np.nonzero(keys == T)[0]
    span = (m + 3) >> 2
    assert places.size >= 3 and np.unique(places // span).size == min(4, places.size)
    taken = need1 - int((keys > T).sum())
    if name == 'mid_m64_need_m':
        assert need1 == m and taken == places.size
    else:
        assert 1 <= taken < places.size                           # the cut is inside the run
    if name == 'mid_m33_need1':
        assert need1 == 1
    if name == 'mid_m101':
        assert m % 4 and m % 8
    assert {sc.BY_NAME[n].claim[True][1] for n in ('mid_m33_need1', 'mid_m255', 'mid_m256')} == {33, 255, 256}


@pytest.mark.parametrize('name', ['crowd_level1_direct', 'crowd_level1_mid', 'crowd_level2', 'crowd_kNm1', 'crowd_kN'])
def test_crowds_split_once_and_the_cut_is_in_the_crowd(name):
    case = sc.BY_NAME[name]
    kth = np.sort(case.scores)[::-1][case.k - 1]
    assert -101 < kth < -50 and (case.scores > -50).sum() < case.k                     # fewer than k candidates are safe
    assert 0.08 < (case.scores > -50).mean() < 0.12
    members, _, _ = kth_bucket(case)
    assert members.size > 256 and members.size == (case.scores < -50).sum()            # the whole crowd in ONE first-level bucket


def test_one_key_cases():
    for name in ('one_key_level1', 'one_key_level2'):
        case = sc.BY_NAME[name]
        kth = np.sort(case.scores)[::-1][case.k - 1]
        copies = (case.scores == kth).sum()
        assert copies > 256 and (case.scores > kth).any() and (case.scores < kth).any()
        assert (case.scores > kth).sum() < case.k < (case.scores > kth).sum() + copies  # the cut inside the copies


def test_full_span():
    for name in ('full_span_cut', 'full_span_all'):
        case = sc.BY_NAME[name]
        keys = f2key(case.scores).astype(np.int64)
        window = int(keys.max() - keys.min())
        assert window == 0xFF000001 and window.bit_length() - 11 == 21                 # sh = 21
        finite = case.scores[np.isfinite(case.scores)]
        assert finite.size == case.N - 2 and finite.min() >= -100.25 and finite.max() <= -99.75
    assert 700 in sc.reference_top_k(sc.BY_NAME['full_span_all'].scores, sc.BY_NAME['full_span_all'].k)      # -inf is elite
    assert 700 not in sc.reference_top_k(sc.BY_NAME['full_span_cut'].scores, sc.BY_NAME['full_span_cut'].k)


def test_signed_zero_cases():
    case = sc.BY_NAME['signed_zeros']
    bits = sc.f2bits(case.scores)
    neg0, pos0 = np.nonzero(bits == 0x80000000)[0], np.nonzero(bits == 0)[0]
    assert neg0.size > case.N // 3 - 2 and pos0.size > case.N // 3 - 2 and (case.scores < 0).sum() == case.N - neg0.size - pos0.size
    ref = sc.reference_top_k(case.scores, case.k)
    cut = ref.max()                                                 # the highest index taken: all taken entries are zeros at or below it
    assert set(ref) <= set(neg0) | set(pos0) and case.k < neg0.size + pos0.size
    for side in (lambda i: i < cut - 3, lambda i: i > cut + 3):     # a -0.0 at a lower index than a +0.0 on each side of the cut
        assert side(neg0).any() and side(pos0).any() and neg0[side(neg0)].min() < pos0[side(pos0)].max()
    pair = sc.BY_NAME['signed_zero_pair']
    bits = sc.f2bits(pair.scores)
    assert pair.N == 64 and (bits == 0x80000000).sum() == 1 and (bits == 0).sum() == 1 and bits[30] == 0x80000000 and bits[31] == 0
    ref = sc.reference_top_k(pair.scores, pair.k)
    assert 30 in ref and 31 not in ref and (pair.scores > 0).sum() == pair.k - 1


def test_nan_case():
    case = sc.BY_NAME['nan']
    bits = sc.f2bits(case.scores)
    nan = np.isnan(case.scores)
    assert 95 <= nan.sum() <= 110 and nan[0] and nan[-1] and (~nan).sum() >= case.k and not np.isneginf(case.scores).any()
    assert (bits[nan] >> 31).min() == 0 and (bits[nan] >> 31).max() == 1 and np.unique(bits[nan] & 0x7FFFFF).size >= 2
    ref = sc.reference_top_k(case.scores, case.k)
    assert not nan[ref].any()
    keys = f2key(case.scores).astype(np.int64)
    assert (keys[nan] == NAN_KEY).all() and keys[~nan].min() > f2key(np.array([-np.inf], np.float32))[0]      # NaN below -inf
    np.testing.assert_array_equal(ref, np.sort(np.lexsort((np.arange(case.N), -keys))[:case.k]))


def test_uncached_cases():
    crowd = sc.BY_NAME['uncached_crowd']
    keys = f2key(crowd.scores)
    in_crowd = crowd.scores < -50
    assert 0.88 < in_crowd.mean() < 0.92 and np.unique(keys[in_crowd] >> 16).size == 1          # the crowd shares its top two key bytes
    bits = sc.f2bits(crowd.scores)
    assert (bits == 0x80000000).any() and (bits == 0).any() and np.isposinf(crowd.scores).any()
    kth = np.sort(crowd.scores)[::-1][crowd.k - 1]
    assert kth < -50 and (~in_crowd).sum() < crowd.k                                            # the cut inside the crowd
    many = sc.BY_NAME['uncached_many_top_bytes']
    assert np.unique(f2key(many.scores[:64]) >> 24).size > 4                                    # past cem_hist_add_clustered's four leader rounds
    for c in UNCACHED:
        assert c.N == 40000


def test_cost_cases_are_crowded_cases():
    for name in sc.COST_CASES:
        assert sc.BY_NAME[name].claim[False][0] >= 1
