"""The host side of the dense factorisation without a GPU (csrc/potrf_plan.hpp: the task tables of both kernels, the plan of a
one-launch call, the workspace layout): tools/potrf_table_check.cpp, compiled with the host compiler, walks every table of its
grid against the kernels' waits (liveness for one queue and for two, exact versions, coverage of A / T / S, end state, the
wave limit, the plan), and the Python restatement of the generator (tools/sim_mega_timing.py build()) is held to the C++ one."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))


@pytest.fixture(scope='module')
def checker(tmp_path_factory):
    cxx = next((c for c in ('c++', 'g++', 'clang++', '/opt/rocm/lib/llvm/bin/clang++') if shutil.which(c)), None)
    assert cxx, 'no host C++ compiler found (tried c++, g++, clang++, /opt/rocm/lib/llvm/bin/clang++)'
    exe = str(tmp_path_factory.mktemp('potrf_table') / 'potrf_table_check')
    subprocess.run([cxx, '-O2', '-std=c++17', os.path.join(ROOT, 'tools', 'potrf_table_check.cpp'), '-o', exe], check=True)
    return exe


def test_every_table_of_the_grid_passes_the_walk(checker):
    r = subprocess.run([checker], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-2000:]
    assert r.stdout.rstrip().endswith('ok')


@pytest.mark.parametrize('inv', [0, 1])
@pytest.mark.parametrize('nbk', [1, 3, 4, 8, 32])
def test_python_restatement_equals_the_generator(checker, nbk, inv):
    import sim_mega_timing as sim
    for batch in (1, 6):
        r = subprocess.run([checker, '--dump', str(nbk), str(inv), str(batch)], capture_output=True, text=True, check=True)
        rows, need = sim.read_dump(r.stdout)
        mine, my_need = sim.table_rows(nbk, inv, batch)
        assert len(need) == nbk and need == my_need
        assert rows == mine
