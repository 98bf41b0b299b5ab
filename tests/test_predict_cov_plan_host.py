"""The covariance additions of the prediction plan (csrc/gpmi_predict_plan.h, HIP-free)
replayed on the host: the chunk row ranges tile the whole working block, the depth
pieces of every split cover the depth once in ascending order, the split choice stays in
range and honours its override, the partial buffer bounds every (tile, piece) index, and
the byte cap rejects a block one tile over it.
tests/host/predict_cov_plan_check.cpp holds the checks; here it is compiled with a plain
host compiler and run."""
import os
import subprocess

from test_ms_sched_host import REPO, CSRC, _host_cxx


def test_predict_cov_plan_host(tmp_path):
    exe = str(tmp_path / 'predict_cov_plan_check')
    subprocess.check_call([_host_cxx(), '-std=c++17', '-O1', '-Wall', '-I', CSRC,
                           os.path.join(REPO, 'tests', 'host', 'predict_cov_plan_check.cpp'),
                           '-o', exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
