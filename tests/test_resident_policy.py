"""The rules that decide which lazily built resident copies a build may evict (voltools_amd/csrc/vt_resident.h), on the host: per-call
pins, fit first, least recently used victims, the spare at its real size, the transient source of a relayout.  The header has no HIP
dependency; tests/resident_policy_driver.cpp is compiled with the host C++ compiler and runs one case per invocation (no GPU)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ['axis2_sequence', 'never_fits', 'lru_order', 'spare_real_size', 'transient_source', 'outside_call']


@pytest.fixture(scope='module')
def driver(tmp_path_factory):
    cxx = shutil.which('c++') or shutil.which('g++') or shutil.which('clang++')
    if not cxx:
        pytest.skip('no host C++ compiler')
    exe = str(tmp_path_factory.mktemp('resident_policy') / 'resident_policy_driver')
    subprocess.run([cxx, '-std=c++17', '-O1', '-Wall', '-I', os.path.join(ROOT, 'voltools_amd', 'csrc'),
                    os.path.join(ROOT, 'tests', 'resident_policy_driver.cpp'), '-o', exe], check=True)
    return exe


@pytest.mark.parametrize('case', CASES)
def test_resident_policy(driver, case):
    r = subprocess.run([driver, case], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
