"""Score vectors for the select (tests/test_select_cases_cpu.py, tests/test_gpu_select_paths.py), each built to send the one-workgroup
cached kernel (cem_select_kernel<true, CROWDED>, csrc/cem_device.h) down one named path, and the value-semantics reference of the elite
set.  A case is (name, N, k, scores float32[N], claim); the claim says, for CROWDED False and True, at which level the bucket select
resolves, how many keys m the k-th key's bucket holds there and how it ends:
  'direct'    m threads rank the bucket's keys against each other (m <= 256; m <= 32 under CROWDED)
  'quarters'  CROWDED only, 32 < m <= 256: the collected list ranked by quarters
  'one_key'   the bucket is one key wide (sh == 0): only ties remain
  'radix'     the population does not fit LDS: byte-wide radix passes on the uncached kernel, whatever the variant (level and m: None)
Vectors with an exact bucket population are built in KEY space (the kernel's order-preserving integers, turned into floats by key2f);
the crowds are built from values, as SafeCemMpc's "return - 100" makes them.  N is a multiple of neither 32, 64 nor 1024 unless a
case says otherwise, so the pad words of the staged key list, the last partial wave and the `i < N` clamps are live.  Importable
without a GPU or torch: NumPy only."""
import collections

import numpy as np

F = np.float32
U = np.uint32

Case = collections.namedtuple('Case', 'name N k scores claim tie signed_zero nan')
# tie: the cut falls inside a run of equal values (the case must tell "lowest index first" from "highest index first")
# signed_zero: the run holds both zeros (the case must tell value order from key order with +0 above -0)


def key2f(keys):
    """float32 of order-preserving keys (sign bit set: a non-negative float's bits with the sign flipped; clear: a negative float's
    bits inverted)."""
    keys = np.asarray(keys, np.uint64).astype(U)
    return np.where(keys & U(0x80000000), keys ^ U(0x80000000), ~keys).astype(U).view(F)


def f2bits(x):
    return np.asarray(x, F).view(U)


def reference_top_k(scores, k):
    """The k largest by VALUE, ties -> lower index (tf.nn.top_k): sorted by (score descending, index ascending) with -0.0 == +0.0 and
    NaN after everything else, -inf included.  Ascending indices.  Without NaN this is oracle.top_k."""
    with np.errstate(invalid='ignore'):                           # (a signalling NaN's cast)
        s = np.asarray(scores, F).astype(np.float64)
    nan = np.isnan(s)
    v = np.where(nan, -np.inf, s)
    order = np.lexsort((np.arange(s.shape[0]), -v, nan))
    return np.sort(order[:k])


def top_k_highest_index_first(scores, k):
    """The same with ties to the HIGHER index: what a tie case must differ from."""
    with np.errstate(invalid='ignore'):                           # (a signalling NaN's cast)
        s = np.asarray(scores, F).astype(np.float64)
    nan = np.isnan(s)
    v = np.where(nan, -np.inf, s)
    order = np.lexsort((-np.arange(s.shape[0]), -v, nan))
    return np.sort(order[:k])


def best_of(scores, elite):
    """Lowest index among the exact maxima of the elite set."""
    e = np.sort(np.asarray(elite))
    return int(e[int(np.argmax(np.asarray(scores, F)[e]))])


def _plant_run(sc, k, before, after):
    """Make the values at ranks k - before .. k + after - 1 (1-based, by value descending) equal to the highest of them: a run of
    before + after equal values with the cut `before` copies in.  The ranks are adjacent, so nothing else moves."""
    with np.errstate(invalid='ignore'):
        order = np.lexsort((np.arange(sc.shape[0]), -sc.astype(np.float64)))       # (NaN sorts last)
    idx = order[k - before:k + after]
    sc[idx] = sc[order[k - before]]
    return idx


def _distinct_keys(rng, n, lo, hi, exclude=None):
    """n distinct keys in [lo, hi), none in [exclude[0], exclude[1])."""
    got = np.zeros(0, np.int64)
    while got.size < n:
        c = rng.integers(lo, hi, size=2 * n + 16, dtype=np.int64)
        if exclude is not None:
            c = c[(c < exclude[0]) | (c >= exclude[1])]
        got = np.unique(np.concatenate([got, c]))
    return rng.permutation(got)[:n]


def _bucket_vector(seed, N, lo_key, hi_key, bucket, m, run, need1):
    """A vector over the key span [lo_key, hi_key] (both present) whose level-0 bucket `bucket` holds exactly m keys: `run` copies of
    one key and m - run distinct others, arranged so that the k-th largest key overall is the need1-th of the bucket and lies in the
    run (the cut takes (run + 1) // 2 copies; all of them when need1 == m).  The bucket's members are scattered over the candidate
    indices, the last one at N - 1; the copies sit at the first, middle and last places of the bucket's members in index order, i.e.
    in different quarters of the list the CROWDED kernel collects wave by wave.  -> (scores, k)"""
    rng = np.random.default_rng(seed)
    window = hi_key - lo_key
    sh = max(0, window.bit_length() - 11)                       # = max(0, 21 - clz(window))
    b_lo = lo_key + (bucket << sh)
    b_hi = b_lo + (1 << sh)
    assert lo_key < b_lo and b_hi <= hi_key and m - run <= (1 << sh) - 1
    take = run if need1 == m else min(need1, (run + 1) // 2)
    above = need1 - take                                        # bucket keys greater than the run's key
    below = m - run - above
    assert above >= 0 and below >= 0
    inner = np.sort(_distinct_keys(rng, m - run + 1, b_lo, b_hi))      # ascending; inner[below] is the run's key
    run_key = inner[below]
    others = np.concatenate([inner[:below], inner[below + 1:]])
    outside = _distinct_keys(rng, N - m - 2, lo_key + 1, hi_key, exclude=(b_lo, b_hi))
    keys = np.empty(N, np.int64)
    members = np.sort(np.concatenate([rng.permutation(N - 1)[:m - 1], [N - 1]]))
    places = np.unique(np.round(np.linspace(0, m - 1, run)).astype(int))
    assert places.size == run
    is_copy = np.zeros(m, bool)
    is_copy[places] = True
    keys[members[is_copy]] = run_key
    keys[members[~is_copy]] = rng.permutation(others)
    rest = np.setdiff1d(np.arange(N), members)
    keys[rest] = np.concatenate([[lo_key, hi_key], outside])[rng.permutation(N - m)]
    k = int((keys >= b_hi).sum()) + need1
    return key2f(keys), k


K_NEG4, K_POS4 = 0x3F7FFFFF, 0xC0800000         # keys of -4.0 and 4.0: a span of 0x81000001, sh = 21
K_ONE, K_TWO = 0xBF800000, 0xC0000000           # keys of 1.0 and 2.0: a span of 2^23, sh = 13


def _crowd(seed, N, width, frac_safe=0.1):
    """SafeCemMpc's scores: unsafe candidates at return - 100 with returns in [0, width), a tenth safe ones spread over [-3, 3]."""
    rng = np.random.default_rng(seed)
    sc = (F(-100.0) + rng.uniform(0.0, width, N).astype(F)).astype(F)
    safe = rng.permutation(N)[:int(round(frac_safe * N))]
    sc[safe] = rng.uniform(-3.0, 3.0, safe.size).astype(F)
    return sc, safe.size


def _cases():
    out = []

    def add(name, N, k, sc, plain, crowded, tie=True, signed_zero=False, nan=False):
        sc = np.ascontiguousarray(sc, F)
        assert sc.shape == (N,) and 1 <= k <= N
        out.append(Case(name, N, int(k), sc, {False: plain, True: crowded}, tie, signed_zero, nan))

    # ---- direct rank at level 0: spread-out scores, 12 keys in the bucket, four of them equal, the cut two copies in
    sc, k = _bucket_vector(1, 1061, K_NEG4, K_POS4, bucket=700, m=12, run=4, need1=6)
    add('direct_level0', 1061, k, sc, (0, 12, 'direct'), (0, 12, 'direct'))

    # ---- between the thresholds at level 0: the plain kernel ranks directly, CROWDED by quarters
    for name, N, m, run, need1, span in [('mid_m33_need1', 1061, 33, 3, 1, (K_ONE, K_TWO)),          # the k-th key is the bucket's largest
                                         ('mid_m255', 4099, 255, 4, 128, (K_NEG4, K_POS4)),
                                         ('mid_m256', 4099, 256, 3, 200, (K_ONE, K_TWO)),
                                         ('mid_m101', 1061, 101, 5, 50, (K_ONE, K_TWO))]:             # 101 % 4 and % 8 != 0: quarters of 26, 26, 26, 23
        sc, k = _bucket_vector(10 + m, N, span[0], span[1], bucket=500, m=m, run=run, need1=need1)
        add(name, N, k, sc, (0, m, 'direct'), (0, m, 'quarters'))
    # need1 == m: the k-th key is the bucket's smallest and the last copy of its run, so every copy is taken (the one variant whose cut
    # lies at the END of a run, not inside it: need1 == m leaves no bucket key outside)
    sc, k = _bucket_vector(64, 1061, K_ONE, K_TWO, bucket=500, m=64, run=3, need1=64)
    add('mid_m64_need_m', 1061, k, sc, (0, 64, 'direct'), (0, 64, 'quarters'), tie=False)

    # ---- split once: a crowd near -100 in ONE first-level bucket (16 units wide there), the cut inside the crowd — fewer than k
    #      candidates are safe.  The crowd's width sets the population of the second-level buckets (0.0078 units each).
    N = 4099
    for name, width, into, plain, crowded in [('crowd_level1_direct', 2.0, 1500, (1, 10, 'direct'), (1, 10, 'direct')),
                                              ('crowd_level1_mid', 0.25, 1500, (1, 114, 'direct'), (1, 114, 'quarters')),
                                              ('crowd_level2', 0.02, 1500, (2, 5, 'one_key'), (2, 5, 'one_key'))]:
        sc, n_safe = _crowd(20, N, width)
        k = n_safe + into
        _plant_run(sc, k, 3, 2)
        add(name, N, k, sc, plain, crowded)

    # ---- one key wide
    rng = np.random.default_rng(30)
    N = 1061
    sc = rng.standard_normal(N).astype(F)                                    # above
    sc[rng.permutation(N)[:200]] = (F(-103.0) - rng.uniform(0, 2, 200).astype(F)).astype(F)      # below
    copies = np.sort(rng.permutation(N)[:300])
    sc[copies] = F(-100.0)
    k = int((sc > F(-100.0)).sum()) + 140
    add('one_key_level2', N, k, sc, (2, 300, 'one_key'), (2, 300, 'one_key'))
    sc = rng.uniform(1.0, 1.2, N).astype(F)                                  # a span below 2^21 keys: sh = 10, the second level is one key wide
    sc[np.sort(rng.permutation(N)[:300])] = F(1.1)
    k = int((sc > F(1.1)).sum()) + 140
    add('one_key_level1', N, k, sc, (1, 300, 'one_key'), (1, 300, 'one_key'))
    add('all_equal', N, 7, np.full(N, 0.5, F), (0, N, 'one_key'), (0, N, 'one_key'))

    # ---- full span: both infinities (window 0xFF000001, sh = 21), everything finite in a band half a unit wide around -100
    rng = np.random.default_rng(40)
    sc = (F(-100.0) + rng.uniform(-0.25, 0.25, N).astype(F)).astype(F)
    sc[5], sc[700] = np.inf, -np.inf
    _plant_run(sc, 400, 3, 2)
    add('full_span_cut', N, 400, sc, (1, 12, 'direct'), (1, 12, 'direct'))
    add('full_span_all', N, N, sc.copy(), (0, 1, 'direct'), (0, 1, 'direct'), tie=False)       # the whole band: -inf is elite

    # ---- signed zeros: -0.0, +0.0, a negative, ... interleaved; the cut inside the zeros
    rng = np.random.default_rng(50)
    sc = (-rng.uniform(0.1, 5.0, N)).astype(F)
    sc[0::3] = F(-0.0)
    sc[1::3] = F(0.0)
    add('signed_zeros', N, 300, sc, (2, 708, 'one_key'), (2, 708, 'one_key'), signed_zero=True)
    sc = (-rng.uniform(0.5, 5.0, 64)).astype(F)                              # N = 64 on purpose: the smallest vector that shows the divergence
    sc[[3, 8, 13, 21, 40, 41, 50, 57, 60, 63]] = rng.uniform(0.5, 5.0, 10).astype(F)
    sc[30], sc[31] = F(-0.0), F(0.0)
    add('signed_zero_pair', 64, 11, sc, (0, 2, 'direct'), (0, 2, 'direct'), signed_zero=True)

    # ---- NaN: both sign bits, two payloads, at index 0, at N - 1 and scattered; no -inf; more than k others
    rng = np.random.default_rng(60)
    sc = np.round(rng.standard_normal(N), 2).astype(F)
    where = np.unique(np.concatenate([[0, N - 1], rng.permutation(N)[:100]]))
    bits = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFC12345], U)
    sc[where] = bits[np.arange(where.size) % 4].view(F)
    _plant_run(sc, 100, 3, 2)
    add('nan', N, 100, sc, (0, 41, 'direct'), (0, 41, 'quarters'), nan=True)

    # ---- k edges on a crowded vector (the lowest two values equal, so that k = N - 1 cuts a tie)
    sc, n_safe = _crowd(70, 4099, 0.25)
    lowest = np.argsort(sc, kind='stable')[:2]
    sc[lowest] = sc[lowest[0]]
    add('crowd_k1', 4099, 1, sc, (0, 10, 'direct'), (0, 10, 'direct'), tie=False)
    add('crowd_kNm1', 4099, 4098, sc.copy(), (1, 112, 'direct'), (1, 112, 'quarters'))
    add('crowd_kN', 4099, 4099, sc.copy(), (1, 112, 'direct'), (1, 112, 'quarters'), tie=False)

    # ---- uncached (N = 40 000: the keys do not fit LDS; select_mode 1 is served by cem_select_kernel<false, false>)
    rng = np.random.default_rng(80)
    N = 40000
    sc = (F(-100.0) + rng.uniform(0.01, 0.49, N).astype(F)).astype(F)       # keys 0x3D38xxxx: one bin in each of the first two radix passes
    safe = rng.permutation(N)[:4000]
    sc[safe] = rng.uniform(-3.0, 3.0, 4000).astype(F)
    sc[safe[0]], sc[safe[1]], sc[safe[2]] = F(-0.0), F(0.0), np.inf
    _plant_run(sc, 5500, 3, 2)
    add('uncached_crowd', N, 5500, sc, (None, None, 'radix'), (None, None, 'radix'))
    sc = np.round(rng.standard_normal(N), 1).astype(F)
    sc[:64] = (np.array([1e-3, 1.0, 100.0, 1e4, -1e-3, -1.0, -100.0, -1e4], F)[np.arange(64) % 8] * (1 + np.arange(64) // 8)).astype(F)
    add('uncached_many_top_bytes', N, 4000, sc, (None, None, 'radix'), (None, None, 'radix'))
    return out


CASES = _cases()
BY_NAME = {c.name: c for c in CASES}
COST_CASES = ('crowd_level1_mid', 'crowd_level2')              # the two crowded cases a 'cost' handle runs (routing in enqueue_select)
