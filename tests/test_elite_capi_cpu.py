"""Elite carry-over (cem_planner_set_elite_carry), the parts of its C ABI that need no GPU: the symbols, what they refuse without a
handle, the sizes of the structs the feature must not have touched, the two kernels' code-object metadata and the policies' constructor
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
from tests import helpers as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('cem_planner_set_elite_carry', 'cem_planner_get_elite_carry', 'cem_planner_elite_store')
INVALID_ARG = 1
# sizeof(cem_config_t), sizeof(cem_layout_t) of ABI 4 as the commit before the feature compiled them (LP64)
CONFIG_BYTES, LAYOUT_BYTES = 712, 136


def test_symbols_are_declared_exported_and_listed(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'cem_mpc.h')).read()
    for name in SYMBOLS:
        assert re.search(r'^int %s\(' % name, hdr, re.M), name
        assert name in _capi.EXPORTED_SYMBOLS
        assert getattr(built_lib, name) is not None
    assert re.search(r'typedef struct \{ int32_t n_keep, across_plans, shift, reserved; \} cem_elite_carry_t;', hdr)
    assert [f[0] for f in _capi.CemEliteCarry._fields_] == ['n_keep', 'across_plans', 'shift', 'reserved'] and C.sizeof(_capi.CemEliteCarry) == 16
    assert re.search(r'#define CEM_ABI_VERSION 4\b', hdr) and built_lib.cem_abi_version() == 4
    mk = open(os.path.join(hp.CSRC, 'Makefile')).read()
    assert mk.count('cem_elite_carry.hip') == 2                                   # a prerequisite and a source of the one link line


def test_null_handle_is_an_invalid_argument_and_writes_nothing(built_lib):
    ec = _capi.CemEliteCarry(n_keep=3, across_plans=0, shift=1, reserved=0)
    assert built_lib.cem_planner_set_elite_carry(None, C.byref(ec)) == INVALID_ARG
    assert built_lib.cem_planner_set_elite_carry(None, None) == INVALID_ARG
    out = _capi.CemEliteCarry(n_keep=7, across_plans=7, shift=7, reserved=7)
    assert built_lib.cem_planner_get_elite_carry(None, C.byref(out)) == INVALID_ARG
    assert (out.n_keep, out.across_plans, out.shift, out.reserved) == (7, 7, 7, 7)
    store = np.full((3, 4, 2), 7.0, np.float32)
    count = C.c_int32(7)
    assert built_lib.cem_planner_elite_store(None, 0, store.ctypes.data_as(C.c_void_p), C.byref(count)) == INVALID_ARG
    assert count.value == 7 and (store == 7.0).all()


def test_config_and_layout_structs_keep_their_sizes(tmp_path):
    assert C.sizeof(_capi.CemConfig) == CONFIG_BYTES and C.sizeof(_capi.CemLayout) == LAYOUT_BYTES
    cc = os.environ.get('CC', 'cc')
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include "cem_mpc.h"\nint main(void) { printf("%zu %zu %zu", sizeof(cem_config_t), sizeof(cem_layout_t), '
                   'sizeof(cem_elite_carry_t)); return 0; }\n')
    exe = tmp_path / 'sz'
    try:
        subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)], check=True, capture_output=True)
    except (OSError, subprocess.CalledProcessError) as e:
        pytest.fail('the header must compile as plain C: %r' % (getattr(e, 'stderr', e),))
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [CONFIG_BYTES, LAYOUT_BYTES, 16]


@pytest.fixture(scope='module')
def carry_isa():
    """The device ISA of csrc/cem_elite_carry.hip, the kernels' own translation unit, with the Makefile's flags (cached like
    helpers.device_assembly).  Without the compiler the test FAILS: the library these tests load was built by it, so its absence is a
    broken set-up, not a reason to let the register check drop out."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    assert os.path.exists(hipcc), 'no hipcc at %s: the carry-over kernels cannot be compiled for their resource check' % hipcc
    h = hashlib.sha256()
    for f in sorted(os.listdir(hp.CSRC)):
        if f.endswith(('.h', '.hip')) or f == 'Makefile':
            h.update(open(os.path.join(hp.CSRC, f), 'rb').read())
    out = '/tmp/cem_elite_isa_%s.s' % h.hexdigest()[:16]
    if not os.path.exists(out):
        r = subprocess.run([hipcc] + hp.makefile_flags() + ['-S', '--cuda-device-only', '-o', out + '.tmp', os.path.join(hp.CSRC, 'cem_elite_carry.hip')],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        os.replace(out + '.tmp', out)
    return open(out).read()


def test_kernels_have_no_spills_no_scratch_no_atomics_and_no_float_arithmetic(carry_isa):
    meta = hp.kernel_meta(carry_isa, r'.', keys=('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size',
                                                 'group_segment_fixed_size'))
    assert sorted(hp.kernel_function_name(n) for n in meta) == ['cem_elite_inject_kernel', 'cem_elite_keep_kernel'], sorted(meta)   # the unit holds these two alone
    bodies = hp.kernel_bodies(carry_isa, r'cem_elite_')
    for name, d in meta.items():
        assert d['vgpr_spill_count'] == 0 and d['sgpr_spill_count'] == 0 and d['private_segment_fixed_size'] == 0, (name, d)
        assert d['group_segment_fixed_size'] == 0, (name, d)                      # the keep's LDS is dynamic (8 k bytes), the inject has none
        assert 0 < d['vgpr_count'] <= 64 and 0 < d['sgpr_count'] <= 100, (name, d)
        body = bodies[name]
        assert not any(re.match(r'(global|flat|ds|buffer)_atomic', l) for l in body), name
        assert not any(re.match(r'scratch_', l) for l in body), name
        # scores are compared as integer keys and actions move as words: no floating-point instruction of any width — but for the
        # compiler's 32-bit integer division (the index arithmetic e / HA, q / AZ), which goes through a float reciprocal
        fp = [l for l in body if re.match(r'v_\w*_f(16|32|64)(_|\b)', l.split()[0])]
        division = [l for l in fp if re.match(r'v_cvt_f32_u32|v_rcp_iflag_f32|v_cvt_u32_f32', l) or (l.startswith('v_mul_f32') and '0x4f7ffffe' in l)]
        assert fp == division, (name, [l for l in fp if l not in division])
        assert any(re.match(r'global_store_dword', l) for l in body), name
    keep = bodies[[n for n in bodies if 'keep' in n][0]]
    assert any(l.startswith('s_barrier') for l in keep) and any(re.match(r'ds_(read|load)', l) for l in keep)


def test_policy_constructor_defaults_are_off():
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    from ethz_safe_learning_amd.simba.policies.safe_cem_mpc import SafeCemMpc
    sig = inspect.signature(CemMpc.__init__).parameters
    assert sig['keep_elites'].default is None and sig['shift_elites'].default is False
    assert 'kwargs' in inspect.signature(SafeCemMpc.__init__).parameters                  # ... which SafeCemMpc passes through
