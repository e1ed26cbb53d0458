"""The option rules of a planner handle on their own (csrc/cem_plan_options.h: admit): tests/native/option_rules_main.cpp, built with
the host compiler under AddressSanitizer + UndefinedBehaviorSanitizer and run as a program of its own — no HIP, no library, no GPU."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_rules_hold_over_the_lattice_of_handle_kinds_and_options(tmp_path):
    cxx = shutil.which(os.environ.get('CXX', 'c++')) or shutil.which('g++') or shutil.which('clang++')
    assert cxx is not None, 'no host C++ compiler (c++ / g++ / clang++, or $CXX)'
    exe = str(tmp_path / 'option_rules')
    r = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-Wall', '-Wextra', '-Werror', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined',
                        '-o', exe, os.path.join(ROOT, 'tests', 'native', 'option_rules_main.cpp')],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=120)
    assert r.returncode == 0 and ' 0 failed' in r.stdout, r.stdout
