"""The dense Cholesky's launch list (csrc/gpmi_dense_plan.h, HIP-free) replayed
symbolically for both panel schedules: every tile receives its operand range once, in
ascending contiguous chunks, from finished tiles, before it is factored, and the
recursive and left-looking schedules cover identical ranges.
tests/host/dense_plan_check.cpp holds the checks; here it is compiled with a plain host
compiler and run."""
import os
import subprocess

from test_ms_sched_host import REPO, CSRC, _host_cxx


def test_dense_plan_host(tmp_path):
    exe = str(tmp_path / 'dense_plan_check')
    subprocess.check_call([_host_cxx(), '-std=c++17', '-Wall', '-I', CSRC,
                           os.path.join(REPO, 'tests', 'host', 'dense_plan_check.cpp'),
                           '-o', exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
