#!/usr/bin/env python
"""Writes profiles/variance_regimes.json (or the path given): the worst values tests/test_gpu_variance_regimes.py measures on an MI355X
— per rung of the variance ladder the relative sd error of every rollout family and the relative var error of forward, and per training
case and tensor the device's gradient error over the fp32 NumPy oracle's own.  The tests fill the numbers in (their module fixture writes
the file named by CEM_VARIANCE_REPORT); this only runs them."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def main():
    import pytest
    out = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.path.join(ROOT, 'profiles', 'variance_regimes.json')
    os.environ['CEM_VARIANCE_REPORT'] = out
    os.chdir(ROOT)
    rc = pytest.main(['tests/test_gpu_variance_regimes.py', '-q', '-s', '-m', 'gpu'])
    print('wrote %s' % out if os.path.exists(out) else 'nothing written')
    return int(rc)


if __name__ == '__main__':
    sys.exit(main())
