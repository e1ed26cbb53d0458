"""What the compiler made of the two lean translation units (hipcc -S --cuda-device-only with the Makefile's own flags; no GPU):
every lean kernel, branchy or straight-line, keeps three workgroups per CU resident (at most 168 VGPRs) with no VGPR spill and no
scratch; the two branchy kernels of csrc/cem_rollout_lean.hip keep the register counts they had before the straight-line form existed;
all six keep the registers, spills, scratch and LDS they had before the two units shared one tile body (csrc/cem_rollout_lean_tile.h);
and the straight-line step loop is what csrc/cem_rollout_lean_straight.hip says it is — the same MFMAs and 16-byte loads per round as
the branchy loop, no scalar load of a kernel argument, fewer vector and scalar instructions."""
import hashlib
import json
import os
import subprocess

import pytest

from tests import helpers as hp
from tests.test_lean_rollout_cpu import MAX_VGPRS, _function_lines, _step_loop

UNITS = {'branchy': 'cem_rollout_lean.hip', 'straight': 'cem_rollout_lean_straight.hip'}
BRANCHY_VGPRS = {'cem_rollout_lean_kernel': 143, 'cem_rollout_lean_seg_kernel': 149}
STRAIGHT_KERNELS = ['cem_rollout_lean_straight_kernel'] * 2 + ['cem_rollout_lean_straight_seg_kernel'] * 2      # {cem, safe} of each


@pytest.fixture(scope='module')
def isa():
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')
    if not os.path.exists(hipcc):
        pytest.skip('no hipcc')
    h = hashlib.sha256()
    for f in sorted(os.listdir(hp.CSRC)):
        if f.endswith(('.h', '.hip')) or f == 'Makefile':
            h.update(open(os.path.join(hp.CSRC, f), 'rb').read())
    out = {}
    for form, unit in UNITS.items():
        path = '/tmp/cem_lean_%s_isa_%s.s' % (form, h.hexdigest()[:16])
        if not os.path.exists(path):
            r = subprocess.run([hipcc] + hp.makefile_flags() + ['-S', '--cuda-device-only', '-o', path + '.tmp', os.path.join(hp.CSRC, unit)],
                               capture_output=True, text=True)
            assert r.returncode == 0, r.stderr[-3000:]
            os.replace(path + '.tmp', path)
        out[form] = open(path).read()
    return out


def test_every_lean_kernel_keeps_three_workgroups_per_cu_without_spills(isa):
    branchy, straight = hp.kernel_meta(isa['branchy'], r'.'), hp.kernel_meta(isa['straight'], r'.')
    assert sorted(hp.kernel_function_name(n) for n in branchy) == sorted(BRANCHY_VGPRS)
    assert sorted(hp.kernel_function_name(n) for n in straight) == STRAIGHT_KERNELS, sorted(straight)
    for name, d in list(branchy.items()) + list(straight.items()):
        assert d['vgpr_count'] <= MAX_VGPRS, (name, d)
        assert d['vgpr_spill_count'] == 0 and d['private_segment_fixed_size'] == 0, (name, d)


def test_the_branchy_kernels_keep_their_register_counts(isa):
    meta = hp.kernel_meta(isa['branchy'], r'.')
    assert {hp.kernel_function_name(n): d['vgpr_count'] for n, d in meta.items()} == BRANCHY_VGPRS


def test_the_lean_kernels_keep_the_registers_of_their_own_tile_bodies(isa):
    """The shared tile body and the shared segment scheduler changed no instruction, so every lean kernel's registers, spills, scratch
    and static LDS are what they were when each unit held a tile body and a scheduler of its own.  The golden is the metadata of
    cem_rollout_lean.hip and cem_rollout_lean_straight.hip at commit 452d227 (the last one with two tile bodies), compiled with the
    Makefile's flags: hipcc <FLAGS without -fPIC -shared> -S --cuda-device-only <unit>, read with helpers.kernel_meta."""
    keys = ('vgpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count', 'private_segment_fixed_size', 'group_segment_fixed_size')
    want = json.load(open(os.path.join(hp.ROOT, 'tests', 'golden', 'lean_rollout_registers.json')))
    assert len(want) == 6
    got = {**hp.kernel_meta(isa['branchy'], r'.', keys), **hp.kernel_meta(isa['straight'], r'.', keys)}
    assert got == want, {k: (want.get(k), got.get(k)) for k in sorted(set(want) | set(got)) if want.get(k) != got.get(k)}


def test_the_straight_line_step_loop(isa):
    """Two steps per round in both forms.  Per round the straight-line loop issues the branchy loop's MFMAs and 16-byte buffer loads
    (weight groups and bias pairs: nothing added, nothing dropped) and its Philox multiplies, loads no kernel argument, and needs
    fewer other vector instructions and fewer scalar instructions than the branchy loop of the same launch form."""
    def count(body, *prefixes):
        return sum(l.startswith(prefixes) for l in body)

    def loops(text, pattern):
        return [_step_loop(lines) for lines in _function_lines(text, pattern).values()]
    for seg in ('lean_kernel', 'lean_seg_kernel'):
        (ref,) = loops(isa['branchy'], 'cem_rollout_' + seg)
        new = loops(isa['straight'], 'cem_rollout_lean_straight_' + seg[5:])
        assert len(new) == 2
        for body in new:
            assert count(body, 'v_mfma') == count(ref, 'v_mfma') == 2 * (4 + 3 * 8 + 8) * 8
            assert count(body, 'buffer_load_dwordx4') == count(ref, 'buffer_load_dwordx4')
            assert count(body, 'v_mad_u64_u32') == count(ref, 'v_mad_u64_u32')
            assert count(body, 's_load', 's_buffer_load') == 0
            assert count(body, 'v_') - count(body, 'v_mfma') < count(ref, 'v_') - count(ref, 'v_mfma')
            assert count(body, 's_') < count(ref, 's_')
            assert count(body, 'v_readlane', 'v_writelane') < count(ref, 'v_readlane', 'v_writelane')
