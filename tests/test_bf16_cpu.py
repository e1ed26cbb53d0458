"""precision='bf16' without a device: the rounding, the host-packed weight image word for word, the status codes of the entry points
that need no GPU — and the bars of tests/test_gpu_bf16.py held on the references alone, with the fp32-accumulating emulation standing
in for the kernel (tests/bf16_cases.py), so that a seed that cannot pass is found here and never on the GPU."""
import ctypes as C

import numpy as np
import pytest

from ethz_safe_learning_amd import _capi, planner
from tests import bf16_cases as bc
from tests import handover_cases as hc

F32 = np.float32


def _rn_bits(bits):
    return int(planner.rn_bf16(np.array([bits], np.uint32).view(F32)).view(np.uint32)[0])


@pytest.mark.parametrize('bits,want', [
    (0x3F808000, 0x3F80), (0x3F818000, 0x3F82),                   # ties: to the even neighbour, down and up
    (0x3F807FFF, 0x3F80), (0x3F808001, 0x3F81),                   # one ulp either side of a tie
    (0x3F817FFF, 0x3F81), (0x3F818001, 0x3F82),
    (0xBF808000, 0xBF80), (0xBF818000, 0xBF82), (0xBF808001, 0xBF81),       # negatives round in magnitude
    (0x00000000, 0x0000), (0x80000000, 0x8000),                   # +-0 keep their sign
    (0x00000001, 0x0000), (0x80000001, 0x8000), (0x00008000, 0x0000), (0x00008001, 0x0001), (0x00018000, 0x0002),   # denormals
    (0x007F8000, 0x0080),                                         # the largest denormals round up into the smallest normal
    (0x3FFF8000, 0x4000), (0x3FFFFFFF, 0x4000),                   # the rounding carries into the exponent: 1.998 -> 2
    (0x7F7EFFFF, 0x7F7F),                                         # just below the largest bf16
    (0x3FC00000, 0x3FC0),                                         # a bf16 value stays what it is
])
def test_rn_bf16_on_bit_patterns(bits, want):
    got = _rn_bits(bits)
    assert got == want << 16, (hex(bits), hex(got), hex(want << 16))


def test_rn_bf16_keeps_shape_and_is_idempotent():
    x = np.random.default_rng(0).standard_normal((7, 5)).astype(F32) * F32(1e3)
    r = planner.rn_bf16(x)
    assert r.shape == x.shape and r.dtype == F32 and np.all((r.view(np.uint32) & 0xFFFF) == 0)
    np.testing.assert_array_equal(planner.rn_bf16(r), r)
    assert np.all(np.abs(r.astype(np.float64) - x) <= np.abs(x) * 2.0 ** -8)          # half an ulp of 8 significand bits
    np.testing.assert_array_equal(planner.rn_bf16(x).view(np.uint32), hc.rn_bf16(x))          # the hand-over suite's own restatement


@pytest.mark.parametrize('O,A', [(60, 2), (100, 12)], ids=['obs60_act2', 'obs100_act12'])
def test_host_packed_image_equals_the_layout_word_for_word(O, A):
    """cem_pack_weights_host on a bf16 configuration: every member's image equals the NumPy restatement of the layout — 2 KB groups
    {a, b} x [64 lanes][8 bf16] in the split kernel's visiting order, zeros past the matrices, 4 KB of zero slack — with the edges of
    the rounding planted among the weights."""
    from ethz_safe_learning_amd import pack_weights_host
    cfg = bc.bf16_config(O, A, 128, L=3, E=2)
    ws = hc.weights(cfg, seed=5, special=True)
    packed = pack_weights_host(cfg, ws).view(np.uint32).reshape(cfg.ensemble_size, -1)
    nfw = (-(-(O + A) // 16) + 3) // 4
    kb_obs = -(-O // 16)
    groups = sum(2 * nfw + 4 * (cfg.n_layers - 1) + 4 * sum(1 for i in range(nfw) if w + 4 * i < kb_obs) for w in range(4))
    assert packed.shape[1] * 4 == groups * 2048 + 4096
    for m, w in enumerate(ws):
        np.testing.assert_array_equal(packed[m], bc.image_bf16(cfg, w), err_msg='member %d' % m)


def test_status_codes_without_a_device():
    """validate() through cem_plan_tiles_host (the status) and the size queries (0 for a configuration that is refused)."""
    lib = _capi.load()
    INVALID_ARG, UNSUPPORTED = 1, 2                                # include/cem_mpc.h enum cem_status

    def status(raw_precision=None, **kw):
        c = planner.to_c_config(bc.bf16_config(60, 2, 128, **kw))
        if raw_precision is not None:
            c.precision = raw_precision
        rc, n = C.c_int32(0), C.c_int32(0)
        return lib.cem_plan_tiles_host(C.byref(c), C.byref(rc), C.byref(n), None, 0), c
    st, c = status()
    assert st == 0 and c.precision == 2
    assert lib.cem_workspace_bytes(C.byref(c)) > 0 and lib.cem_packed_weight_floats(C.byref(c)) > 0
    st, c = status(units=129)
    assert st == UNSUPPORTED and lib.cem_workspace_bytes(C.byref(c)) == 0
    st, c = status(activation='tanh')
    assert st == UNSUPPORTED and lib.cem_workspace_bytes(C.byref(c)) == 0
    st, c = status(raw_precision=3)
    assert st == INVALID_ARG and lib.cem_workspace_bytes(C.byref(c)) == 0
    st, c = status(raw_precision=-1)
    assert st == INVALID_ARG
    st, c = status()
    assert lib.cem_batch_workspace_bytes(C.byref(c), 4) == 0                       # batch handles stay fp32-only
    c.precision = 0
    assert lib.cem_batch_workspace_bytes(C.byref(c), 4) > 0


# ---- the bars of the GPU tests, held on the references alone ---------------------------------------------------------------------
@pytest.mark.parametrize('dims', bc.SHAPES, ids=bc.SHAPE_IDS)
@pytest.mark.parametrize('order', [0, 1, 2])
def test_trajectory_bars_with_the_fp32_emulation_in_the_kernels_place(dims, order):
    """GPU test 2 with emu32 for the kernel: RMS(stand-in - emulation) <= 0.05 x RMS(emulation - fp64 oracle) and the max condition, at
    every step."""
    _, _, _, _, emu, ref64 = bc.traj_case(dims)
    ratios = bc.check_rounding_model(bc.traj_stand_in(dims, order), emu, ref64, 'obs %d' % dims[0])
    M = [bc.rms(emu[:, t] - ref64[:, t]) for t in range(emu.shape[1])]
    print('obs %d: RMS(emulation - fp64) per step %s; ratios %s' % (dims[0], ' '.join('%.2e' % m for m in M[1:]), ' '.join('%.4f' % r for r in ratios[1:])))
    assert 1e-6 < M[1] < 1e-3 and M[-1] > M[1], M              # the rounding is visible and grows along the horizon


@pytest.mark.parametrize('variant', ['cem', 'safe'])
@pytest.mark.parametrize('O,A', [(60, 2), (100, 12)], ids=['obs60', 'obs100'])
@pytest.mark.parametrize('order', [0, 1, 2])
def test_score_bars_with_the_fp32_emulation_in_the_kernels_place(O, A, variant, order):
    """GPU test 3 with emu32 for the kernel: the exclusion cap, the admissible outcomes of the near-threshold candidates and the two
    conditions on the rest, and the two quantile conditions on the flip-free candidates."""
    ratio, near, med, p90 = bc.check_scores(bc.score_stand_in(O, A, variant, order), bc.score_case(O, A, variant), 'obs %d %s' % (O, variant))
    print('obs %d %s: ratio %.4f, %.1f %% of the candidates near a threshold; over the flip-free ones median ratio %.4f, 90th percentile ratio %.4f' % (
        O, variant, ratio, 100 * near, med, p90))


@pytest.mark.parametrize('variant', ['cem', 'safe'])
@pytest.mark.parametrize('dims', bc.SHAPES, ids=bc.SHAPE_IDS)
@pytest.mark.parametrize('order', [0, 1, 2])
def test_plan_bars_with_the_fp32_emulation_in_the_kernels_place(dims, variant, order):
    """GPU test 5 with emu32 for the kernel: the whole plan under the two emulations agrees at the split test's bars — for three
    stand-ins whose bf16 ties fall differently: this fixes the seeds of the GPU test (bf16_cases.PLAN_SEED)."""
    bc.check_plan(bc.plan_stand_in(dims, variant, order), bc.plan_case(dims, variant)['ref'], 'obs %d %s' % (dims[0], variant))


@pytest.mark.parametrize('dims', bc.SHAPES, ids=bc.SHAPE_IDS)
def test_exact_cases_do_not_depend_on_the_summation_order(dims):
    """The premise of GPU test 1: on bf16_cases.exact_problem the float32-accumulating emulation equals the float64 one bit for bit in
    every chunk order (every sum is exact), the states stay finite and move, and the bf16 rounding of the operands does bite."""
    O, A, U = dims
    pb = bc.exact_problem(O, A, U, E=5, seed=O)
    s0, acts, eps = bc.exact_inputs(O, A, 40, 3, seed=O + 1)
    args = (s0, acts, pb['weights'], bc.members_of(40, 5), pb['inputs_min'], pb['inputs_max'], eps)
    with bc.emulating(bc.emu64):
        rt, rm, rs = bc.unfold_with_moments(*args)
    assert np.all(np.isfinite(rt)) and np.abs(rt[:, 1:] - rt[:, :-1]).max() > 0.1 and np.any(planner.rn_bf16(rt[:, 1:]) != rt[:, 1:])
    import functools
    for order in range(3):
        with bc.emulating(functools.partial(bc.emu32, order=order)):
            t, m, s = bc.unfold_with_moments(*args)
        np.testing.assert_array_equal(t, rt); np.testing.assert_array_equal(m, rm)
    plain = bc.unfold_with_moments(*args)[0]
    assert np.abs(plain - rt).max() > 1e-3                     # ... against the unrounded network


def test_emulations_agree_with_the_oracle_where_nothing_is_rounded():
    """On bf16-representable weights and inputs whose every activation stays bf16-representable (one layer, power-of-two products)
    the emulations are the oracle's own network; and the context manager restores the oracle."""
    from oracle import cem_oracle as o
    rng = np.random.default_rng(1)
    W = np.zeros((8, 8), F32); W[rng.permutation(8), np.arange(8)] = 2.0
    w = dict(W=[W], b=[np.zeros(8, F32)], W_mu=W.copy(), b_mu=np.zeros(8, F32), W_var=W.copy(), b_var=np.full(8, -4.0, F32))
    x = (rng.integers(-8, 9, (5, 8)) / 8.0).astype(F32)
    want = o.gaussian_dist_mlp(x, w)
    for f in (bc.emu64, bc.emu32):
        got = f(x, w)
        np.testing.assert_array_equal(got[0], want[0]); np.testing.assert_allclose(got[1], want[1], rtol=1e-6)
    saved = o.gaussian_dist_mlp
    with pytest.raises(RuntimeError):
        with bc.emulating(bc.emu64):
            assert o.gaussian_dist_mlp is bc.emu64
            raise RuntimeError
    assert o.gaussian_dist_mlp is saved


# ---- the build: what the tile rule and the residency table of cem_capi.hip rest on ---------------------------------------------------
def _bf16_unit_assembly():
    """cem_rollout_bf16.hip compiled to assembly with the Makefile's flags (cached under /tmp on the hash of the device sources).
    Skips the calling test where there is no hipcc."""
    import hashlib, os, subprocess
    from tests import helpers as hp
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    h = hashlib.sha256()
    for f in sorted(os.listdir(hp.CSRC)):
        if f.endswith(('.h', '.hip')) or f == 'Makefile':
            h.update(open(os.path.join(hp.CSRC, f), 'rb').read())
    out = '/tmp/cem_bf16_isa_%s.s' % h.hexdigest()[:16]
    if not os.path.exists(out):
        r = subprocess.run([hipcc] + hp.makefile_flags() + ['-S', '--cuda-device-only', '-o', out + '.tmp', os.path.join(hp.CSRC, 'cem_rollout_bf16.hip')],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        os.replace(out + '.tmp', out)
    return open(out).read()


def test_bf16_rollout_kernels_fit_the_residency_their_tile_rule_assumes():
    """cem_rollout_bf16.hip compiled to assembly with the Makefile's flags (cached under /tmp on the hash of the device sources): all 16
    instantiations, no spilled VGPR anywhere, no scratch and no more VGPRs than kBf16Resident assumes (512 / resident workgroups) in
    the planning instantiations; the products are bf16 MFMAs (one per chunk and output block: 2 x (2 + 4 + 4) in the unrolled stages
    of the one-chunk kernel), nothing falls back to fp32 MFMAs, and the operands are rounded by the hardware conversion."""
    import re
    from tests import helpers as hp
    isa = _bf16_unit_assembly()
    meta = hp.kernel_meta(isa, r'cem_rollout_bf16_kernelILi\dELi\dELi\dEE')
    assert len(meta) == 16, sorted(meta)
    resident = {1: (4, 3, 2, 2), 2: (3, 2, 2, 2)}            # cem_capi.hip kBf16Resident[nfw - 1][rc - 1]
    for name, d in meta.items():
        rc, nfw, mode = (int(x) for x in re.search(r'ILi(\d)ELi(\d)ELi(\d)E', name).groups())
        assert d['vgpr_spill_count'] == 0, (name, d)
        if mode == 0:
            assert d['private_segment_fixed_size'] == 0, (name, d)
            assert d['vgpr_count'] <= 512 // resident[nfw][rc - 1], (name, d)
    assert hp.kernel_meta(isa, r'cem_pack_bf16_kernel')
    m = re.search(r'^(_Z23cem_rollout_bf16_kernelILi1ELi1ELi0EEv13RolloutParams):.*?\n(.*?)^\.Lfunc_end', isa, re.M | re.S)
    ins = [l.split(';')[0].strip() for l in m.group(2).splitlines() if l.strip() and not l.lstrip().startswith((';', '.'))]
    assert sum(1 for l in ins if l.startswith('v_mfma_f32_16x16x32_bf16')) >= 2 * (2 + 4 + 4)
    assert not any(l.startswith('v_mfma_f32_16x16x4_f32') for l in ins), 'the bf16 kernel must not fall back to fp32 MFMAs'
    assert any(l.startswith('v_cvt_pk_bf16_f32') for l in ins), 'operands are rounded to nearest even by the hardware conversion'
    assert not any(l.startswith('scratch_') for l in ins)


def test_bf16_rollout_kernels_keep_their_register_counts():
    """Every cem_rollout_bf16_kernel instantiation keeps the registers, spills, scratch and LDS it had when the tile rule's residency row
    (cem_capi.hip kBf16Resident: 512 / VGPRs of the planning instantiations, 113 145 171 205 | 155 185 221 253) was measured.  The
    golden is the metadata of cem_rollout_bf16.hip at commit 52f6ae7 (the last one with a tile body of its own), compiled with the
    Makefile's flags: hipcc <FLAGS without -fPIC -shared> -S --cuda-device-only cem_rollout_bf16.hip, read with helpers.kernel_meta."""
    import json, os
    from tests import helpers as hp
    keys = ('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size', 'group_segment_fixed_size')
    want = json.load(open(os.path.join(hp.ROOT, 'tests', 'golden', 'bf16_rollout_registers.json')))
    assert len(want) == 16
    got = hp.kernel_meta(_bf16_unit_assembly(), r'cem_rollout_bf16_kernelILi\dELi\dELi\dEE', keys)
    assert got == want, {k: (want.get(k), got.get(k)) for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)}


def test_the_forced_generic_rollout_is_refused(monkeypatch):
    """CEM_FORCE_GENERIC_ROLLOUT (a diagnostic) routes a handle to the generic fp32 kernel; bf16x3 lets it, being fp32-grade.  A bf16
    configuration is refused: its arithmetic is its contract."""
    lib = _capi.load()
    c = planner.to_c_config(bc.bf16_config(60, 2, 128))
    assert lib.cem_workspace_bytes(C.byref(c)) > 0
    monkeypatch.setenv('CEM_FORCE_GENERIC_ROLLOUT', '1')
    rc, n = C.c_int32(0), C.c_int32(0)
    assert lib.cem_plan_tiles_host(C.byref(c), C.byref(rc), C.byref(n), None, 0) == 2          # CEM_ERR_UNSUPPORTED
    assert lib.cem_workspace_bytes(C.byref(c)) == 0
    c.precision = 1
    assert lib.cem_plan_tiles_host(C.byref(c), C.byref(rc), C.byref(n), None, 0) == 0
