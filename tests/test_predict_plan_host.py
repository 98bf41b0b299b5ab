"""The prediction's launch list, chunking and workspace sizes (csrc/gpmi_predict_plan.h,
HIP-free) replayed symbolically: every tile of the working block receives each operand
range once, from finished tiles, before its diagonal step; the chunks cover the test
points exactly; the workspace sizes bound every index.
tests/host/predict_plan_check.cpp holds the checks; here it is compiled with a plain host
compiler and run."""
import os
import subprocess

from test_ms_sched_host import REPO, CSRC, _host_cxx


def test_predict_plan_host(tmp_path):
    exe = str(tmp_path / 'predict_plan_check')
    subprocess.check_call([_host_cxx(), '-std=c++17', '-Wall', '-I', CSRC,
                           os.path.join(REPO, 'tests', 'host', 'predict_plan_check.cpp'),
                           '-o', exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
