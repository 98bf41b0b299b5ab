"""The cell plan of the tapered Matérn assembly (csrc/gpmi_cell_plan.h, HIP-free) on the
host: every point lies in the cell its coordinates say, the cell starts are the prefix sum
of the populations, each cell lists its points in ascending index, the locality order is a
permutation that keeps cells together, points closer than the cutoff in every dimension lie
in the same or adjacent cells, a grid with too many cells is coarsened, and non-finite
points, a width that is not positive or a grid that cannot be coarsened give no plan.
tests/host/cell_plan_check.cpp holds the checks; here it is compiled with a plain host
compiler and run."""
import os
import subprocess

from test_ms_sched_host import REPO, CSRC, _host_cxx


def test_cell_plan_host(tmp_path):
    exe = str(tmp_path / 'cell_plan_check')
    subprocess.check_call([_host_cxx(), '-std=c++17', '-O1', '-Wall', '-I', CSRC,
                           os.path.join(REPO, 'tests', 'host', 'cell_plan_check.cpp'),
                           '-o', exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
