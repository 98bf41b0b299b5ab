"""The cell rule for a new point of the sparse prediction's cross assembly
(csrc/gpmi_cell_plan.h: cross_cell_coord, cross_cell_range; HIP-free, compiled by the host
and by the kernels alike) on the host: for plans in d = 1, 2, 3 and new points inside, on
the faces of, just outside and far outside the training box, every training point within
the cutoff in every dimension lies in a visited cell, the visited cells are in range and
distinct, a far point visits none, and +-inf / NaN / huge coordinates neither overflow nor
index out of range. tests/host/cross_plan_check.cpp holds the checks; here it is compiled
with a plain host compiler and run."""
import os
import subprocess

from test_ms_sched_host import REPO, CSRC, _host_cxx


def test_cross_plan_host(tmp_path):
    exe = str(tmp_path / 'cross_plan_check')
    subprocess.check_call([_host_cxx(), '-std=c++17', '-O1', '-Wall', '-I', CSRC,
                           os.path.join(REPO, 'tests', 'host', 'cross_plan_check.cpp'),
                           '-o', exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
