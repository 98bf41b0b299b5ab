"""The sampler's plan (csrc/gpmi_sample_plan.h, HIP-free) replayed on the host: the depth
pieces of every row tile cover its triangular depth once in ascending order with the
diagonal tile in the last piece, the work list names every piece once, deepest first, the
partial buffer bounds every (piece, draw tile) index, and the piece depth stays in range,
honours its override and the cap on partial tiles.
tests/host/sample_plan_check.cpp holds the checks; here it is compiled with a plain host
compiler and run."""
import os
import subprocess

from test_ms_sched_host import REPO, CSRC, _host_cxx


def test_sample_plan_host(tmp_path):
    exe = str(tmp_path / 'sample_plan_check')
    subprocess.check_call([_host_cxx(), '-std=c++17', '-O1', '-Wall', '-I', CSRC,
                           os.path.join(REPO, 'tests', 'host', 'sample_plan_check.cpp'),
                           '-o', exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
