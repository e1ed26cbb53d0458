"""Population schedule and mean candidate (cem_planner_set_population_schedule, cem_planner_set_mean_candidate), the parts of their C
ABI that need no GPU: the symbols, what they refuse without a handle, the sizes of the structs the feature must not have touched, the
new kernel's code-object metadata and the policies' constructor defaults."""
import ctypes as C
import hashlib
import inspect
import os
import re
import subprocess

import pytest

from ethz_safe_learning_amd import _capi
from tests import helpers as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('cem_planner_set_population_schedule', 'cem_planner_get_population_schedule', 'cem_planner_iteration_plan',
           'cem_planner_set_mean_candidate', 'cem_planner_get_mean_candidate')
PLAN_FIELDS = ['n_samples', 'chunks_per_tile', 'n_tiles', 'n_segments', 'n_pinned', 'launches', 'rollout_path', 'reserved']
INVALID_ARG = 1
# sizeof(cem_config_t), sizeof(cem_layout_t) of ABI 4 as the commit before the feature compiled them (LP64); cem_iteration_plan_t
CONFIG_BYTES, LAYOUT_BYTES, PLAN_BYTES = 712, 136, 32


def test_symbols_are_declared_exported_and_listed(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'cem_mpc.h')).read()
    for name in SYMBOLS:
        assert re.search(r'^int %s\(' % name, hdr, re.M), name
        assert name in _capi.EXPORTED_SYMBOLS
        assert getattr(built_lib, name) is not None
    assert re.search(r'typedef struct \{ int32_t %s; \} cem_iteration_plan_t;' % ', '.join(PLAN_FIELDS), hdr)
    assert [f[0] for f in _capi.CemIterationPlan._fields_] == PLAN_FIELDS and C.sizeof(_capi.CemIterationPlan) == PLAN_BYTES
    assert re.search(r'#define CEM_ABI_VERSION 4\b', hdr) and built_lib.cem_abi_version() == 4
    mk = open(os.path.join(hp.CSRC, 'Makefile')).read()
    assert mk.count('cem_population.hip') == 2                                    # a prerequisite and a source of the one link line
    assert mk.count('cem_elite_carry.hip') == 2


def test_null_handle_is_an_invalid_argument_and_writes_nothing(built_lib):
    n = (C.c_int32 * 3)(64, 48, 32)
    assert built_lib.cem_planner_set_population_schedule(None, n, 3) == INVALID_ARG
    assert built_lib.cem_planner_set_population_schedule(None, None, 0) == INVALID_ARG
    out, on = (C.c_int32 * 3)(7, 7, 7), C.c_int32(7)
    assert built_lib.cem_planner_get_population_schedule(None, out, 3, C.byref(on)) == INVALID_ARG
    assert list(out) == [7, 7, 7] and on.value == 7
    ip = _capi.CemIterationPlan(*([7] * 8))
    assert built_lib.cem_planner_iteration_plan(None, 0, C.byref(ip)) == INVALID_ARG
    assert [getattr(ip, f) for f in PLAN_FIELDS] == [7] * 8
    assert built_lib.cem_planner_set_mean_candidate(None, 1) == INVALID_ARG
    assert built_lib.cem_planner_get_mean_candidate(None, C.byref(on)) == INVALID_ARG
    assert on.value == 7


def test_config_and_layout_structs_keep_their_sizes(tmp_path):
    assert C.sizeof(_capi.CemConfig) == CONFIG_BYTES and C.sizeof(_capi.CemLayout) == LAYOUT_BYTES
    cc = os.environ.get('CC', 'cc')
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include "cem_mpc.h"\nint main(void) { printf("%zu %zu %zu", sizeof(cem_config_t), sizeof(cem_layout_t), '
                   'sizeof(cem_iteration_plan_t)); return 0; }\n')
    exe = tmp_path / 'sz'
    try:
        subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)], check=True, capture_output=True)
    except (OSError, subprocess.CalledProcessError) as e:
        pytest.fail('the header must compile as plain C: %r' % (getattr(e, 'stderr', e),))
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [CONFIG_BYTES, LAYOUT_BYTES, PLAN_BYTES]


def _unit_isa(unit, tag):
    """The device ISA of one translation unit of csrc with the Makefile's flags (cached like helpers.device_assembly).  Without the
    compiler the test FAILS: the library these tests load was built by it."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    assert os.path.exists(hipcc), 'no hipcc at %s: %s cannot be compiled for its resource check' % (hipcc, unit)
    h = hashlib.sha256()
    for f in sorted(os.listdir(hp.CSRC)):
        if f.endswith(('.h', '.hip')) or f == 'Makefile':
            h.update(open(os.path.join(hp.CSRC, f), 'rb').read())
    out = '/tmp/cem_%s_isa_%s.s' % (tag, h.hexdigest()[:16])
    if not os.path.exists(out):
        r = subprocess.run([hipcc] + hp.makefile_flags() + ['-S', '--cuda-device-only', '-o', out + '.tmp', os.path.join(hp.CSRC, unit)],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        os.replace(out + '.tmp', out)
    return open(out).read()


def test_the_unit_holds_one_kernel_without_spills_scratch_lds_or_atomics():
    isa = _unit_isa('cem_population.hip', 'population')
    meta = hp.kernel_meta(isa, r'.', keys=('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size',
                                           'group_segment_fixed_size'))
    assert [hp.kernel_function_name(n) for n in meta] == ['cem_mean_candidate_kernel'], sorted(meta)
    (name, d), = meta.items()
    assert d['vgpr_spill_count'] == 0 and d['sgpr_spill_count'] == 0 and d['private_segment_fixed_size'] == 0, d
    assert d['group_segment_fixed_size'] == 0, d
    assert 0 < d['vgpr_count'] <= 64 and 0 < d['sgpr_count'] <= 100, d
    body = hp.kernel_bodies(isa, r'cem_mean_candidate')[name]
    assert not any(re.match(r'(global|flat|ds|buffer)_atomic', l) for l in body)
    assert not any(re.match(r'(scratch_|ds_)', l) for l in body)
    # the only floating-point work is the max and the min — but for the compiler's 32-bit integer division (q / AZ), which goes
    # through a float reciprocal
    fp = [l for l in body if re.match(r'v_\w*_f(16|32|64)(_|\b)', l.split()[0])]
    division = [l for l in fp if re.match(r'v_cvt_f32_u32|v_rcp_iflag_f32|v_cvt_u32_f32', l) or (l.startswith('v_mul_f32') and '0x4f7ffffe' in l)]
    clip = [l for l in fp if re.match(r'v_(max|min|med3|pk_max|pk_min)\w*_f32', l)]
    assert sorted(fp) == sorted(division + clip), [l for l in fp if l not in division and l not in clip]
    assert clip and any(re.match(r'global_store_dword', l) for l in body)


def test_the_carry_over_unit_keeps_exactly_its_two_kernels():
    isa = _unit_isa('cem_elite_carry.hip', 'elite_unit')
    meta = hp.kernel_meta(isa, r'.')
    assert sorted(hp.kernel_function_name(n) for n in meta) == ['cem_elite_inject_kernel', 'cem_elite_keep_kernel'], sorted(meta)


def test_policy_constructor_defaults_are_off():
    from ethz_safe_learning_amd.planner import PlannerConfig
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    from ethz_safe_learning_amd.simba.policies.safe_cem_mpc import SafeCemMpc
    sig = inspect.signature(CemMpc.__init__).parameters
    assert sig['population_decay'].default is None and sig['min_population'].default is None and sig['mean_candidate'].default is False
    assert 'kwargs' in inspect.signature(SafeCemMpc.__init__).parameters                  # ... which SafeCemMpc passes through
    f = PlannerConfig.__dataclass_fields__
    assert f['population'].default == () and f['mean_candidate'].default is False
