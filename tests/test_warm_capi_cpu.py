"""Warm start, the parts that need no GPU: the C ABI additions (declared, exported, mirrored), argument checks that return before any
device call, the workspace growth, and the NumPy restatement of CEM_INIT_SHIFT against hand-written arrays."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from ethz_safe_learning_amd import _capi
from ethz_safe_learning_amd.planner import PlannerConfig, ScorerConfig, shift_distribution, to_c_config, warm_sigma_floor
from tests import helpers as hp
from tests import warm_cases as wc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ['cem_planner_set_warm_start', 'cem_planner_set_initial_distribution', 'cem_planner_set_init_mode', 'cem_planner_reset_carry',
       'cem_planner_get_carry', 'cem_planner_set_carry_slots']


def _cfg(**kw):
    base = dict(obs_dim=60, act_dim=2, ensemble_size=5, particles=5, n_samples=2000, horizon=30, n_elite=200, iterations=5,
                scorer=ScorerConfig(goal_slice=(3, 19), cost_kinds=[(22, 38, 0.2)]), act_low=[-1, -1], act_high=[1, 1])
    base.update(kw)
    return PlannerConfig(**base)


def test_new_symbols_are_declared_exported_and_listed(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'cem_mpc.h')).read()
    for name in NEW:
        assert re.search(r'\bint %s\s*\(' % name, hdr), name
        assert hasattr(built_lib, name) and name in _capi.EXPORTED_SYMBOLS, name
    assert re.search(r'CEM_INIT_COLD = 0, CEM_INIT_EXPLICIT = 1, CEM_INIT_SHIFT = 2', hdr)
    assert (_capi.CEM_INIT_COLD, _capi.CEM_INIT_EXPLICIT, _capi.CEM_INIT_SHIFT) == (0, 1, 2)
    assert built_lib.cem_abi_version() == 4 and _capi.CEM_ABI_VERSION == 4


def test_warm_start_struct_has_the_headers_size(tmp_path):
    assert C.sizeof(_capi.CemWarmStart) == 3 * 4 + 4 * _capi.CEM_MAX_ACT
    cc = os.environ.get('CC', 'cc')
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "cem_mpc.h"\nint main(void) { printf("%zu %zu %zu", sizeof(cem_warm_start_t), '
                   'offsetof(cem_warm_start_t, sigma_floor), sizeof(cem_config_t)); return 0; }\n')
    exe = tmp_path / 'sz'
    try:
        subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)], check=True, capture_output=True)
    except (OSError, subprocess.CalledProcessError) as e:
        pytest.fail('the header must compile as plain C: %r' % (getattr(e, 'stderr', e),))
    size, off, cfg_size = map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split())
    assert size == C.sizeof(_capi.CemWarmStart) and off == _capi.CemWarmStart.sigma_floor.offset
    assert cfg_size == C.sizeof(_capi.CemConfig)             # cem_config_t kept its fields


def test_null_handles_return_invalid_arg_without_a_device_call(built_lib):
    lib = built_lib
    ws = _capi.CemWarmStart(shift=1)
    buf = (C.c_float * 64)()
    v = C.c_int32()
    sl = (C.c_int32 * 2)(0, 1)
    assert lib.cem_planner_set_warm_start(None, C.byref(ws)) == 1
    assert lib.cem_planner_set_initial_distribution(None, 0, buf, buf) == 1
    assert lib.cem_planner_set_init_mode(None, 0, 0) == 1
    assert lib.cem_planner_reset_carry(None, -1) == 1
    assert lib.cem_planner_get_carry(None, 0, buf, buf, C.byref(v)) == 1
    assert lib.cem_planner_set_carry_slots(None, 2, sl) == 1


@pytest.mark.parametrize('shape', [dict(), dict(ensemble_size=15, particles=5, n_samples=150, horizon=8, n_elite=15, iterations=10),
                                   dict(ensemble_size=15, particles=45, n_samples=500, horizon=8, n_elite=20, iterations=9, variant='safe'),
                                   dict(n_samples=20000, n_elite=2000)], ids=['B2', 'cem_mpc', 'safe_cem_mpc', 'B4'])
def test_workspace_grows_by_the_carry_and_explicit_buffers_only(built_lib, shape):
    """The two new buffers are the layout's last (make_layout takes them behind every old one, so no old offset moves), each
    slots x 2 x H x A floats rounded up to the 256-byte grain: the workspace is at least that large and still a multiple of the grain,
    and what was added stays within slots x 4 x H x A floats plus the two roundings."""
    cfg = _cfg(**shape)
    cc = to_c_config(cfg)
    HA4 = cfg.horizon * cfg.act_dim * 4
    for mb in (0, 8):
        total = built_lib.cem_batch_workspace_bytes(C.byref(cc), mb) if mb else built_lib.cem_workspace_bytes(C.byref(cc))
        if mb and total == 0:
            continue                                       # (B4 is outside what batch handles serve)
        slots = mb or 1
        added = 2 * ((slots * 2 * HA4 + 255) & ~255)
        assert total % 256 == 0 and total > added
        assert added <= slots * 4 * HA4 + 2 * 255
    src = open(os.path.join(ROOT, 'ethz_safe_learning_amd', 'csrc', 'cem_capi.hip')).read()
    body = src[src.index('Layout make_layout('):src.index('size_t max_tiles_of(')]
    new = 'l.carry = take(nb * 2 * d.H * d.A * 4); l.expl = take(nb * 2 * d.H * d.A * 4);'
    assert body.index('l.ms_colmean = take(') < body.index(new) < body.index('l.total = o;')
    assert 'take(' not in body[body.index(new) + len(new):]                # nothing is taken behind them


H, A = 5, 2
MU = np.arange(10, dtype=np.float32).reshape(H, A) / 16            # mu[t, a] = (2 t + a) / 16
SG = np.array([[.5, .4], [.3, .05], [.2, .6], [.01, .3], [.7, .02]], np.float32)
MU0, SG0, FL = np.array([.25, -.25], np.float32), np.array([1., 2.], np.float32), np.array([.1, .25], np.float32)


@pytest.mark.parametrize('s,tail,rule,mu_want,sg_want', [
    (1, 0, 0, [[.125, .1875], [.25, .3125], [.375, .4375], [.5, .5625], [.25, -.25]], [[1, 2]] * 5),
    (1, 1, 1, [[.125, .1875], [.25, .3125], [.375, .4375], [.5, .5625], [.5, .5625]], [[.3, .25], [.2, .6], [.1, .3], [.7, .25], [1, 2]]),
    (3, 0, 1, [[.375, .4375], [.5, .5625], [.25, -.25], [.25, -.25], [.25, -.25]], [[.1, .3], [.7, .25], [1, 2], [1, 2], [1, 2]]),
    (3, 1, 0, [[.375, .4375], [.5, .5625], [.5, .5625], [.5, .5625], [.5, .5625]], [[1, 2]] * 5),
    (4, 0, 0, [[.5, .5625], [.25, -.25], [.25, -.25], [.25, -.25], [.25, -.25]], [[1, 2]] * 5),
    (4, 1, 1, [[.5, .5625]] * 5, [[.7, .25], [1, 2], [1, 2], [1, 2], [1, 2]]),
])
def test_shift_restatement_against_hand_written_arrays(s, tail, rule, mu_want, sg_want):
    for fn in (lambda: shift_distribution(MU, SG, MU0, SG0, shift=s, tail=tail, sigma_rule=rule, sigma_floor=FL),
               lambda: wc.shift(MU, SG, MU0, SG0, s, tail, rule, FL)):
        m, g = fn()
        assert m.dtype == np.float32 and g.dtype == np.float32
        np.testing.assert_array_equal(m, np.array(mu_want, np.float32))
        np.testing.assert_array_equal(g, np.array(sg_want, np.float32))


def test_shift_restatement_rejects_a_shift_outside_the_horizon():
    for s in (0, H, -1):
        with pytest.raises(ValueError):
            shift_distribution(MU, SG, MU0, SG0, shift=s)


def test_sigma_floor_is_the_fp32_product():
    fl = warm_sigma_floor(_cfg(act_low=[-1, -3], act_high=[1, 3]), 0.25)
    np.testing.assert_array_equal(fl, np.float32(0.25) * np.array([1, 3], np.float32))


# ---- nothing else moved: the planning kernels' register budgets are what they were before warm start -----------------------------
@pytest.fixture(scope='module')
def isa():
    """The device assembly, compiled with the Makefile's own flags (the recipe and cache file tests/test_isa_cpu.py uses)."""
    return hp.device_assembly()


def test_planning_kernels_keep_their_register_counts(isa):
    """Warm start lives in the plan's first kernel alone.  tests/golden/kernel_registers_before_warm_start.json records vgpr_count, spilled
    VGPRs (none anywhere) and scratch of every other kernel as the code-object metadata gave them for the device sources of the commit
    before the feature, compiled with these flags; they must still be exactly those.  What may stand beside them is said by name: the
    plan's first kernel, the trainer's and the forward pass's kernels (function names that begin with cem_train_ / cem_trainer_), and the
    kernels added since, listed in helpers.KERNELS_SINCE_WARM_START — stricter than the earlier rule, which admitted every mangled name
    that held the letters `train` (`constraint` and `constrained` among them)."""
    import json
    want = json.load(open(os.path.join(ROOT, 'tests', 'golden', 'kernel_registers_before_warm_start.json')))
    got = hp.kernel_meta(isa, r'.')
    assert len(want) > 40 and all(d['vgpr_spill_count'] == 0 for d in want.values())
    for name, d in want.items():
        assert name in got, name
        assert got[name] == d, (name, got[name], d)
    fn = {n: hp.kernel_function_name(n) for n in got}
    admitted = {n for n in got if fn[n].startswith(('cem_train_', 'cem_trainer_')) or fn[n] in hp.KERNELS_SINCE_WARM_START}
    assert set(got) - set(want) == {'_Z15cem_init_kernel10InitParams'} | admitted
    assert set(hp.KERNELS_SINCE_WARM_START) <= set(fn.values())
    init = got['_Z15cem_init_kernel10InitParams']
    assert init['vgpr_spill_count'] == 0 and init['private_segment_fixed_size'] == 0, init
