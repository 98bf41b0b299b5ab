"""The band path's shapes and sizes (csrc/gpmi_band_plan.h, HIP-free): the cyclic
reduction's level list, the capacity groups' sizes per eta, the look-ahead SYR2K's tile
orders, the split-K tile count and the eta chunking. tests/host/band_plan_check.cpp
holds the checks; here it is compiled with a plain host compiler and run."""
import os
import subprocess

from test_ms_sched_host import REPO, CSRC, _host_cxx


def test_band_plan_host(tmp_path):
    exe = str(tmp_path / 'band_plan_check')
    subprocess.check_call([_host_cxx(), '-std=c++17', '-Wall', '-I', CSRC,
                           os.path.join(REPO, 'tests', 'host', 'band_plan_check.cpp'),
                           '-o', exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
