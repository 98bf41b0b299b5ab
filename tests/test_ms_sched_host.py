"""The multi-shift CG's host scheduler (csrc/gpmi_ms_sched.h, HIP-free) against a CPU
model of the device: tests/host/ms_sched_check.cpp holds the scenarios, the invariants
and the expected outcomes; here it is compiled with a plain host compiler and run."""
import os
import shutil
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, 'gaussian-process-param-estimation_amd', 'csrc')


def _host_cxx():
    for cxx in ('c++', 'g++', '/opt/rocm/llvm/bin/clang++', '/opt/rocm/lib/llvm/bin/clang++'):
        path = shutil.which(cxx)
        if path:
            return path
    raise AssertionError('no host C++ compiler (c++, g++ or ROCm clang++)')


def test_ms_sched_host(tmp_path):
    exe = str(tmp_path / 'ms_sched_check')
    subprocess.check_call([_host_cxx(), '-std=c++17', '-Wall', '-I', CSRC,
                           os.path.join(REPO, 'tests', 'host', 'ms_sched_check.cpp'),
                           '-o', exe])
    run = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert run.returncode == 0, run.stdout + run.stderr
