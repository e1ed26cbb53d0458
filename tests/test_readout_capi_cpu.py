"""Plan read-out (cem_planner_set_plan_readout), the parts of its C ABI that need no GPU: the symbols, what they refuse without a
handle, the sizes of the structs the feature must not have touched, the tracker's code-object metadata and the policies' constructor
defaults."""
import ctypes as C
import hashlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from ethz_safe_learning_amd import _capi
from ethz_safe_learning_amd.planner import PlannerConfig, PlanReadout, config_key, to_c_config
from tests import helpers as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('cem_planner_set_plan_readout', 'cem_planner_get_plan_readout', 'cem_planner_plan_readout', 'cem_planner_graph_nodes')
INVALID_ARG = 1
# sizeof(cem_config_t), sizeof(cem_layout_t) of ABI 4 as the commit before the feature compiled them (LP64)
CONFIG_BYTES, LAYOUT_BYTES = 712, 136


def test_symbols_are_declared_exported_and_listed(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'cem_mpc.h')).read()
    for name in SYMBOLS:
        assert re.search(r'^int %s\(' % name, hdr, re.M), name
        assert name in _capi.EXPORTED_SYMBOLS
        assert getattr(built_lib, name) is not None
    assert re.search(r'typedef struct \{ float score; int32_t candidate, iteration, flags; \} cem_plan_readout_t;', hdr)
    assert [f[0] for f in _capi.CemPlanReadout._fields_] == ['score', 'candidate', 'iteration', 'flags'] and C.sizeof(_capi.CemPlanReadout) == 16
    assert re.search(r'#define CEM_ABI_VERSION 4\b', hdr) and built_lib.cem_abi_version() == 4
    mk = open(os.path.join(hp.CSRC, 'Makefile')).read()
    assert mk.count('cem_plan_readout.hip') == 2                                  # a prerequisite and a source of the one link line


def test_null_handle_is_an_invalid_argument_and_writes_nothing(built_lib):
    assert built_lib.cem_planner_set_plan_readout(None, 1) == INVALID_ARG
    on = C.c_int32(7)
    assert built_lib.cem_planner_get_plan_readout(None, C.byref(on)) == INVALID_ARG and on.value == 7
    assert built_lib.cem_planner_graph_nodes(None, C.byref(on)) == INVALID_ARG and on.value == 7
    head = _capi.CemPlanReadout(score=7.0, candidate=7, iteration=7, flags=7)
    seq = np.full((4, 2), 7.0, np.float32)
    ret = np.full(5, 7.0, np.float32)
    cnt = np.full(4, 7, np.int32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    assert built_lib.cem_planner_plan_readout(None, 0, C.byref(head), vp(seq), vp(ret), vp(cnt)) == INVALID_ARG
    assert (head.score, head.candidate, head.iteration, head.flags) == (7.0, 7, 7, 7)
    assert (seq == 7.0).all() and (ret == 7.0).all() and (cnt == 7).all()


def test_config_and_layout_structs_keep_their_sizes(tmp_path):
    assert C.sizeof(_capi.CemConfig) == CONFIG_BYTES and C.sizeof(_capi.CemLayout) == LAYOUT_BYTES
    cc = os.environ.get('CC', 'cc')
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include "cem_mpc.h"\nint main(void) { printf("%zu %zu %zu", sizeof(cem_config_t), sizeof(cem_layout_t), '
                   'sizeof(cem_plan_readout_t)); return 0; }\n')
    exe = tmp_path / 'sz'
    try:
        subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)], check=True, capture_output=True)
    except (OSError, subprocess.CalledProcessError) as e:
        pytest.fail('the header must compile as plain C: %r' % (getattr(e, 'stderr', e),))
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [CONFIG_BYTES, LAYOUT_BYTES, 16]


def test_the_option_is_part_of_the_cache_key_and_not_of_the_c_config():
    from ethz_safe_learning_amd.planner import ScorerConfig
    kw = dict(obs_dim=12, act_dim=2, ensemble_size=5, particles=5, n_samples=64, horizon=5, n_elite=8, iterations=3,
              scorer=ScorerConfig(goal_slice=(3, 7)), act_low=[-1, -1], act_high=[1, 1], units=32)
    off, on = PlannerConfig(**kw), PlannerConfig(plan_readout=True, **kw)
    assert off.plan_readout is False
    assert config_key(off) != config_key(on)
    assert bytes(to_c_config(off)) == bytes(to_c_config(on))
    assert PlanReadout._fields == ('sequence', 'score', 'candidate', 'iteration', 'particle_returns', 'cost_counts', 'flags')


@pytest.fixture(scope='module')
def readout_isa():
    """The device ISA of csrc/cem_plan_readout.hip, the tracker's own translation unit, with the Makefile's flags (cached like
    helpers.device_assembly).  Without the compiler the test FAILS: the library these tests load was built by it, so its absence is a
    broken set-up, not a reason to let the register check drop out."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    assert os.path.exists(hipcc), 'no hipcc at %s: the tracker cannot be compiled for its resource check' % hipcc
    h = hashlib.sha256()
    for f in sorted(os.listdir(hp.CSRC)):
        if f.endswith(('.h', '.hip')) or f == 'Makefile':
            h.update(open(os.path.join(hp.CSRC, f), 'rb').read())
    out = '/tmp/cem_readout_isa_%s.s' % h.hexdigest()[:16]
    if not os.path.exists(out):
        r = subprocess.run([hipcc] + hp.makefile_flags() + ['-S', '--cuda-device-only', '-o', out + '.tmp', os.path.join(hp.CSRC, 'cem_plan_readout.hip')],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        os.replace(out + '.tmp', out)
    return open(out).read()


def test_the_tracker_has_no_spills_no_scratch_no_global_atomics_and_no_float_arithmetic(readout_isa):
    meta = hp.kernel_meta(readout_isa, r'.', keys=('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size',
                                                   'group_segment_fixed_size'))
    assert sorted(hp.kernel_function_name(n) for n in meta) == ['cem_plan_track_kernel'], sorted(meta)         # the unit holds this one alone
    (name, d), = meta.items()
    print('cem_plan_track_kernel:', d)
    assert d['vgpr_spill_count'] == 0 and d['sgpr_spill_count'] == 0 and d['private_segment_fixed_size'] == 0, d
    assert d['group_segment_fixed_size'] == 16, d                                 # wave_min [4]: the minimum over the workgroup
    assert 0 < d['vgpr_count'] <= 32 and 0 < d['sgpr_count'] <= 100, d
    body = hp.kernel_bodies(readout_isa, r'cem_plan_track')[name]
    assert not any(re.match(r'(global|flat|buffer)_atomic', l) for l in body)
    assert not any(re.match(r'ds_\w*(add|sub|min|max|cmpst|inc|dec|and|or|xor)_', l) for l in body)          # (nor LDS ones: shuffles and four words)
    assert not any(re.match(r'scratch_', l) for l in body)
    # scores are compared as integer keys, everything else moves as words or is counted: no floating-point instruction of any width
    fp = [l for l in body if re.match(r'v_\w*_f(16|32|64)(_|\b)', l.split()[0])]
    assert fp == [], fp
    assert any(re.match(r'global_store_dword', l) for l in body)
    assert any(l.startswith('s_barrier') for l in body) and any(re.match(r'ds_(read|load)', l) for l in body)


def test_policy_constructor_defaults_are_off():
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    from ethz_safe_learning_amd.simba.policies.safe_cem_mpc import SafeCemMpc
    sig = inspect.signature(CemMpc.__init__).parameters
    assert sig['plan_readout'].default is False and sig['replan_every'].default == 1
    assert 'kwargs' in inspect.signature(SafeCemMpc.__init__).parameters                  # ... which SafeCemMpc passes through
