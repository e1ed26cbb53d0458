"""The arithmetic claim behind the split-product rollout (csrc/cem_rollout_split.h), checked on the CPU in numpy:
an fp32 number is the EXACT sum of three bf16 pieces (round-to-nearest-even split), every bf16 x bf16 product is exact in fp32, and
the six products with i + j <= 2 reproduce w * x to within 2^-22 of |w * x| — the scale of one fp32 rounding.  (The truncation
split of the first version is exact too but only reaches 2^-21: its pieces shrink by 2^-7 each, not 2^-8.)"""
import numpy as np


def rn_bf16(x):
    """cem_rn_bf16_bits: round to nearest even at 8 significand bits, as a float32 whose low 16 bits are zero."""
    u = np.asarray(x, np.float32).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32)


def split3(x, rn=True):
    """cem_split3_bits: the three pieces as float32 arrays that are bf16 values."""
    x = np.asarray(x, np.float32)
    top = rn_bf16 if rn else (lambda v: (v.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32))
    a0 = top(x)
    r1 = x - a0
    a1 = top(r1)
    a2 = r1 - a1
    return a0, a1, a2


def _samples():
    rng = np.random.default_rng(0)
    x = np.concatenate([rng.standard_normal(200000), rng.standard_normal(50000) * 1e-6, rng.standard_normal(50000) * 1e6,
                        np.array([0.0, -0.0, 1.0, -1.0, 3.3e38, -3.3e38, 1.1754944e-38, 2.0 ** -100, 1.0 + 2.0 ** -23, 1.0 - 2.0 ** -24])]).astype(np.float32)
    return x


def test_three_bf16_pieces_are_an_exact_split():
    x = _samples()
    a0, a1, a2 = split3(x)
    for a in (a0, a1, a2):
        assert np.all((a.view(np.uint32) & np.uint32(0xFFFF)) == 0), 'a piece is not a bf16 value'
    # exact in fp64 (every piece and the sum are representable): no rounding anywhere
    np.testing.assert_array_equal(a0.astype(np.float64) + a1.astype(np.float64) + a2.astype(np.float64), x.astype(np.float64))
    # and the fp32 subtractions that produce the pieces were exact too
    np.testing.assert_array_equal((x - a0) - a1, a2)


def test_six_leading_products_carry_the_product_to_fp32_grade():
    rng = np.random.default_rng(1)
    w = (rng.standard_normal(300000) * rng.choice([1e-3, 1.0, 30.0], 300000)).astype(np.float32)
    x = (rng.standard_normal(300000) * rng.choice([1e-2, 1.0, 5.0], 300000)).astype(np.float32)
    ws, xs = split3(w), split3(x)
    exact = w.astype(np.float64) * x.astype(np.float64)
    kept = np.zeros_like(exact)
    for i in range(3):
        for j in range(3):
            p = ws[i].astype(np.float64) * xs[j].astype(np.float64)
            # a bf16 x bf16 product has at most 16 significant bits: exact in an fp32 accumulator
            np.testing.assert_array_equal(p, (ws[i] * xs[j]).astype(np.float64))
            if i + j <= 2:
                kept += p
    rel = np.abs(kept - exact) / np.maximum(np.abs(exact), 1e-300)
    assert rel.max() <= 2.0 ** -22, rel.max()
    # the truncation split, for comparison: exact as a split, but its dropped products reach 2^-21
    wt, xt = split3(w, rn=False), split3(x, rn=False)
    kept_t = sum(wt[i].astype(np.float64) * xt[j].astype(np.float64) for i in range(3) for j in range(3) if i + j <= 2)
    rel_t = np.abs(kept_t - exact) / np.maximum(np.abs(exact), 1e-300)
    assert 2.0 ** -22 < rel_t.max() <= 2.0 ** -20
    # what an fp32 multiply itself loses, for scale
    assert (np.abs((w * x).astype(np.float64) - exact) / np.maximum(np.abs(exact), 1e-300)).max() <= 2.0 ** -24 * 1.0001


def test_dot_products_of_split_operands_match_fp32_dot_products():
    """A 128-term dot product (one hidden unit): six-product form accumulated in fp32 vs the fp64 value, next to plain fp32."""
    rng = np.random.default_rng(2)
    W = (rng.standard_normal((512, 128)) / np.sqrt(128)).astype(np.float32)
    X = np.maximum(rng.standard_normal((512, 128)), 0).astype(np.float32)
    exact = (W.astype(np.float64) * X.astype(np.float64)).sum(axis=1)
    ws, xs = split3(W), split3(X)
    acc = np.zeros(512, np.float32)
    for (i, j) in ((2, 0), (1, 1), (0, 2), (1, 0), (0, 1), (0, 0)):      # the kernel's order: smallest terms first
        for k0 in range(0, 128, 32):                                      # one MFMA adds 32 exact products to the accumulator
            acc = (acc.astype(np.float64) + (ws[i][:, k0:k0 + 32].astype(np.float64) * xs[j][:, k0:k0 + 32].astype(np.float64)).sum(axis=1)).astype(np.float32)
    plain = np.zeros(512, np.float32)
    for k in range(128):
        plain = plain + W[:, k] * X[:, k]
    scale = np.abs(W.astype(np.float64) * X.astype(np.float64)).sum(axis=1)
    e_split, e_plain = np.abs(acc - exact) / scale, np.abs(plain - exact) / scale
    assert e_split.max() <= 4e-7 and e_split.max() <= 2.0 * max(e_plain.max(), 6e-8), (e_split.max(), e_plain.max())


# ---- the packed weight stream of the split kernel (pack_member_chunked), consumed the way cem_rollout_split.h consumes it ----------------
def _bf16_planes_to_f64(words16):
    return (np.asarray(words16, np.uint32) << 16).view(np.float32).astype(np.float64)


def _perm(w, phi):                                        # cem_split_perm
    return w if phi == 0 else (phi - 1 if phi - 1 < w else phi)


import pytest


@pytest.mark.parametrize('obs_dim,act_dim,n_layers,units', [(60, 2, 4, 128), (100, 12, 3, 128), (23, 3, 2, 48), (64, 2, 2, 128)])
def test_split_weight_stream_reproduces_the_network(obs_dim, act_dim, n_layers, units):
    """Every 6 KB group of every wave's stream, read with the lane map of v_mfma_f32_16x16x32_bf16 (lane 16 q + i: output feature
    16 G + i, k slots s = 0..7 = input features 16 (2 F + s / 4) + 4 q + s % 4), holds the three bf16 pieces of exactly the weight the
    kernel multiplies there — their sum is the fp32 weight bit for bit — in the order the kernel visits the chunks (layer 0 ascending,
    hidden / heads stages own chunk first), and one step consumes the whole stream once."""
    from ethz_safe_learning_amd import PlannerConfig, ScorerConfig, pack_weights_host
    from oracle import cem_oracle as o
    E = 2
    pb = o.synthetic_problem(obs_dim=obs_dim, act_dim=act_dim, ensemble_size=E, units=units, n_layers=n_layers, seed=11)
    cfg = PlannerConfig(obs_dim=obs_dim, act_dim=act_dim, ensemble_size=E, particles=2, n_samples=64, horizon=4, n_elite=4, iterations=2,
                        n_layers=n_layers, units=units, scorer=ScorerConfig(goal_slice=(0, 2)), act_low=[-1] * act_dim, act_high=[1] * act_dim,
                        precision='bf16x3')
    packed = pack_weights_host(cfg, pb['weights']).view(np.uint16)
    D = obs_dim + act_dim
    nfw = ((D + 15) // 16 + 3) // 4
    kb_obs = (obs_dim + 15) // 16
    nch0 = 2 * nfw
    groups = [nch0 + 4 * (n_layers - 1) + 4 * sum(1 for i in range(nfw) if w + 4 * i < kb_obs) for w in range(4)]
    stride16 = packed.size // E
    assert stride16 >= sum(groups) * 3072
    lane = np.arange(64); qq, ii = lane >> 4, lane & 15
    for m in range(E):
        wts = pb['weights'][m]
        pos = m * stride16
        for w in range(4):
            def check(W, in_dim, out_dim, F, Ga, Gb):
                nonlocal pos
                g = packed[pos:pos + 3072].reshape(6, 64, 8)
                for ab, G in ((0, Ga), (1, Gb)):
                    val = sum(_bf16_planes_to_f64(g[3 * ab + pl]) for pl in range(3))          # [64 lanes][8 slots]
                    for s in range(8):
                        k = 16 * (2 * F + (s >> 2)) + 4 * qq + (s & 3)
                        oo = 16 * G + ii
                        ok = (k < in_dim) & (oo < out_dim)
                        ref = np.where(ok, W[np.minimum(k, in_dim - 1), np.minimum(oo, out_dim - 1)].astype(np.float64), 0.0)
                        np.testing.assert_array_equal(val[:, s], ref)
                pos += 3072
            for P in range(nch0):
                check(wts['W'][0], D, units, P, 2 * w, 2 * w + 1)
            for l in range(1, n_layers):
                for P in range(4):
                    check(wts['W'][l], units, units, _perm(w, P), 2 * w, 2 * w + 1)
            for i in range(nfw):
                Fo = w + 4 * i
                if Fo >= kb_obs:
                    continue
                for P in range(4):
                    F = _perm(w, P)
                    g = packed[pos:pos + 3072].reshape(6, 64, 8)
                    for ab, Wh in ((0, wts['W_mu']), (1, wts['W_var'])):
                        val = sum(_bf16_planes_to_f64(g[3 * ab + pl]) for pl in range(3))
                        for s in range(8):
                            k = 16 * (2 * F + (s >> 2)) + 4 * qq + (s & 3)
                            oo = 16 * Fo + ii
                            ok = (k < units) & (oo < obs_dim)
                            ref = np.where(ok, Wh[np.minimum(k, units - 1), np.minimum(oo, obs_dim - 1)].astype(np.float64), 0.0)
                            np.testing.assert_array_equal(val[:, s], ref)
                    pos += 3072
            assert pos - m * stride16 == sum(groups[:w + 1]) * 3072
