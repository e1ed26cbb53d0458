"""Time-correlated action noise (cem_planner_set_action_noise, CEM_NOISE_MIXED), the parts of its C ABI that need no GPU: the symbols,
what they refuse without a handle, the sizes of the structs the feature must not have touched, the mix kernel's code-object metadata and
the policies' constructor defaults."""
import ctypes as C
import hashlib
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

from ethz_safe_learning_amd import _capi, planner
from tests import helpers as hp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ('cem_planner_set_action_noise', 'cem_planner_get_action_noise', 'cem_planner_action_noise_dev')
INVALID_ARG = 1
# sizeof(cem_config_t), sizeof(cem_layout_t) of ABI 4 as the commit before the feature compiled them (LP64)
CONFIG_BYTES, LAYOUT_BYTES = 712, 136


def test_symbols_are_declared_exported_and_listed(built_lib):
    hdr = open(os.path.join(ROOT, 'include', 'cem_mpc.h')).read()
    for name in SYMBOLS:
        assert re.search(r'^int %s\(' % name, hdr, re.M), name
        assert name in _capi.EXPORTED_SYMBOLS
        assert getattr(built_lib, name) is not None
    assert re.search(r'enum cem_action_noise \{ CEM_NOISE_WHITE = 0, CEM_NOISE_MIXED = 1 \}', hdr)
    assert (_capi.CEM_NOISE_WHITE, _capi.CEM_NOISE_MIXED) == (0, 1)
    assert planner.ACTION_NOISES == ('white', 'powerlaw', 'ar1')
    assert re.search(r'#define CEM_ABI_VERSION 4\b', hdr) and built_lib.cem_abi_version() == 4


def test_null_handle_is_an_invalid_argument_and_writes_nothing(built_lib):
    M = np.eye(4, dtype=np.float32)
    mp = M.ctypes.data_as(C.c_void_p)
    for kind, ptr in ((0, None), (1, mp), (1, None), (0, mp), (2, mp), (-1, None)):
        assert built_lib.cem_planner_set_action_noise(None, kind, ptr) == INVALID_ARG
    kind = C.c_int32(7)
    out = np.full((4, 4), 7.0, np.float32)
    assert built_lib.cem_planner_get_action_noise(None, C.byref(kind), out.ctypes.data_as(C.c_void_p)) == INVALID_ARG
    assert kind.value == 7 and (out == 7.0).all()
    ptr, n = C.c_void_p(5), C.c_size_t(7)
    assert built_lib.cem_planner_action_noise_dev(None, C.byref(ptr), C.byref(n)) == INVALID_ARG
    assert (ptr.value, n.value) == (5, 7)


def test_python_wrapper_refuses_before_any_call():
    class Stub:
        cfg = type('cfg', (), dict(horizon=8))
    with pytest.raises(ValueError):
        planner.CemPlanner.set_action_noise(Stub(), 'pink', 1.0)       # (no handle is touched: the kind is checked first)
    with pytest.raises(ValueError):
        planner.CemPlanner.set_action_noise(Stub(), np.eye(7))          # a matrix of another horizon
    with pytest.raises(ValueError):
        planner.CemPlanner.set_action_noise(Stub(), 'ar1', 1.0)


def test_config_and_layout_structs_keep_their_sizes(tmp_path):
    assert C.sizeof(_capi.CemConfig) == CONFIG_BYTES and C.sizeof(_capi.CemLayout) == LAYOUT_BYTES
    cc = os.environ.get('CC', 'cc')
    src = tmp_path / 'sz.c'
    src.write_text('#include <stdio.h>\n#include "cem_mpc.h"\nint main(void) { printf("%zu %zu %d %d", sizeof(cem_config_t), sizeof(cem_layout_t), '
                   '(int)CEM_NOISE_WHITE, (int)CEM_NOISE_MIXED); return 0; }\n')
    exe = tmp_path / 'sz'
    try:
        subprocess.run([cc, '-I', os.path.join(ROOT, 'include'), '-o', str(exe), str(src)], check=True, capture_output=True)
    except (OSError, subprocess.CalledProcessError) as e:
        pytest.fail('the header must compile as plain C: %r' % (getattr(e, 'stderr', e),))
    got = list(map(int, subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()))
    assert got == [CONFIG_BYTES, LAYOUT_BYTES, 0, 1]


@pytest.fixture(scope='module')
def mix_isa():
    """The device ISA of csrc/cem_noise_mix.hip, the kernel's own translation unit, with the Makefile's flags (cached like
    helpers.device_assembly).  Without the compiler the test FAILS: the library these tests load was built by it, so its absence is a
    broken set-up, not a reason to let the register check drop out."""
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    assert os.path.exists(hipcc), 'no hipcc at %s: the mix kernel cannot be compiled for its resource check' % hipcc
    h = hashlib.sha256()
    for f in sorted(os.listdir(hp.CSRC)):
        if f.endswith(('.h', '.hip')) or f == 'Makefile':
            h.update(open(os.path.join(hp.CSRC, f), 'rb').read())
    out = '/tmp/cem_mix_isa_%s.s' % h.hexdigest()[:16]
    if not os.path.exists(out):
        r = subprocess.run([hipcc] + hp.makefile_flags() + ['-S', '--cuda-device-only', '-o', out + '.tmp', os.path.join(hp.CSRC, 'cem_noise_mix.hip')],
                           capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-3000:]
        os.replace(out + '.tmp', out)
    return open(out).read()


def test_mix_kernel_has_no_spills_no_scratch_and_separate_multiply_and_add(mix_isa):
    meta = hp.kernel_meta(mix_isa, r'.')
    assert [hp.kernel_function_name(n) for n in meta] == ['cem_mix_action_noise_kernel'], sorted(meta)     # the unit holds this kernel alone
    (name, d), = meta.items()
    assert d['vgpr_spill_count'] == 0 and d['private_segment_fixed_size'] == 0, d
    assert 0 < d['vgpr_count'] <= 128, d
    block = re.search(r'\.name:\s+%s\s*\n(.*?)(?=\n\s+- \.|\namdhsa\.target|\Z)' % re.escape(name), mix_isa, re.S).group(0)
    assert re.search(r'\.sgpr_spill_count:\s+0\b', block), 'SGPRs spilled into vector lanes'
    body = hp.kernel_bodies(mix_isa, r'cem_mix_action_noise_kernel')[name]
    assert not any(re.match(r'(global|flat|ds|buffer)_atomic', l) for l in body), 'no atomics of any kind'
    # the dot products: products and sums rounded separately.  They are the code that reads xi back from LDS a quad at a time, so: cut
    # the kernel into its straight-line pieces (at every branch); a piece with such a read multiplies and adds, and fuses nothing.  (The
    # fused multiply-adds of cem_normal4, which turn Philox words into uniforms as in every other sampler, sit in the piece that WRITES
    # xi; how many of them the compiler makes is not this test's business.)
    pieces, cur = [], []
    for l in body:
        cur.append(l)
        if re.match(r's_c?branch', l):
            pieces.append(cur)
            cur = []
    pieces.append(cur)
    dots = [p for p in pieces if any(re.match(r'ds_(read|load)_b128', l) for l in p)]
    assert dots, 'no piece reads xi quads from LDS'
    for p in dots:
        fused = [l for l in p if re.match(r'v_(pk_)?(fma|mad|fmac|mac|dot)\w*_f(32|16)', l)]
        assert not fused, fused
        assert any(l.startswith(('v_pk_mul_f32', 'v_mul_f32')) for l in p) and any(l.startswith(('v_pk_add_f32', 'v_add_f32')) for l in p), p


def test_policy_constructor_defaults_are_none():
    from ethz_safe_learning_amd.simba.policies.cem_mpc import CemMpc
    from ethz_safe_learning_amd.simba.policies.safe_cem_mpc import SafeCemMpc
    sig = inspect.signature(CemMpc.__init__).parameters
    assert sig['noise_beta'].default is None and sig['noise_rho'].default is None
    assert 'kwargs' in inspect.signature(SafeCemMpc.__init__).parameters                  # ... which SafeCemMpc passes through
