"""What the option setters of a planner handle ANSWER, against the answers recorded from the library as it was before the rules were
gathered in csrc/cem_plan_options.h (tests/golden/option_statuses.json, written by scripts/record_option_statuses.py).

Seven handle kinds at the smoke shape (CemMpc, SafeCemMpc and cost objective; select_mode 2 and 3; world_size 2; a batch handle of 2),
every ordered pair of the option moves, every ordered triple of the elite / schedule / mean-candidate moves (their rule is three-way),
cem_planner_comm_init behind every move.  Every status must be the recorded one; a final comm_init compares as "CEM_ERR_UNSUPPORTED or
not" (an admitted call goes on into RCCL — here the shared-memory stand-in of tests/test_gpu_multirank.py).  The recorder binds that
stand-in for its whole process, so it runs as a process of its own."""
import importlib.util
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCRIPT = os.path.join(ROOT, 'scripts', 'record_option_statuses.py')
GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'option_statuses.json')


def _recorder():
    spec = importlib.util.spec_from_file_location('record_option_statuses', SCRIPT)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_recorded_file_covers_what_it_should():
    rec, want = _recorder(), json.load(open(GOLDEN))
    assert list(want['kinds']) == [k[0] for k in rec.KINDS] and want['moves'] == rec.MOVES
    keys = ['>'.join(s) for s in rec.sequences()]
    seen = set()
    for name, kd in want['kinds'].items():
        assert list(kd['statuses']) == keys, name
        seen |= {ch for st in kd['statuses'].values() for ch in st}
    assert seen == {'0', '2', '7'}                      # CEM_OK, CEM_ERR_UNSUPPORTED, CEM_ERR_STATE (comm_init on a batch handle)
    assert [want['kinds'][k]['select_mode'] for k in ('cem', 'select2', 'select3')] == [1, 2, 3]
    cem, safe = want['kinds']['cem']['statuses'], want['kinds']['safe']['statuses']
    # one recorded refusal per rule the smoke shape can reach ("The option rules")
    assert want['kinds']['world2']['statuses']['tail>readout'] == '22'                       # one rank
    assert cem['mixed>comm'] == '02' and cem['-mixed>comm'] == '00'                          # no communicator
    assert want['kinds']['select2']['statuses']['softmax>keep1'] == '22'                     # the one-workgroup select
    assert want['kinds']['batch2']['statuses']['pop32>keep1x'] == '22' and want['kinds']['batch2']['statuses']['keep1>mean'] == '02'   # a single-state handle
    assert want['kinds']['cost']['statuses']['tail>budget'] == '22' and cem['budget>tail'] == '20'      # the variant
    assert safe['tail>budget'] == '02' and safe['budget>tail'] == '02'                       # one m
    assert cem['keep12>pop13>mean'] == '002' and cem['mean>pop13>keep12'] == '002' and cem['keep12>pop32>mean'] == '000'   # the inject's rows
    assert cem['softmax>comm'] == '00'                                                       # the inherited asymmetry: comm_init admits the softmax refit


@pytest.mark.gpu
def test_every_setter_answers_as_recorded(tmp_path):
    rec = _recorder()
    r = subprocess.run(['make', '-C', os.path.join(ROOT, 'tests', 'fakes')], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and os.path.exists(rec.FAKE), r.stdout
    out = str(tmp_path / 'option_statuses.json')
    r = subprocess.run([sys.executable, SCRIPT, '--out', out], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stdout
    got, want = rec.comparable(json.load(open(out))), rec.comparable(json.load(open(GOLDEN)))
    assert list(got) == list(want)
    for name in want:
        assert got[name]['select_mode'] == want[name]['select_mode'], name
        diff = {s: (got[name]['statuses'].get(s), st) for s, st in want[name]['statuses'].items() if got[name]['statuses'].get(s) != st}
        assert not diff and len(got[name]['statuses']) == len(want[name]['statuses']), (name, 'sequence: (answered, recorded)', diff)
