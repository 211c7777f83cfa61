"""
The slab planner of the final stage (brx_plan_final in badread_amd/csrc/brx_finplan.h: host arithmetic, no HIP call)
checked on the CPU: tests/native/finplan_check.hip is compiled with hipcc and run here.  The header takes the read
state (RS) from brx_kernels.h, so the program is built as plain C++ against the emulation header of
tests/native/emu -- as tests/emu_engine.py builds the driver -- instead of compiling every kernel for a device it never uses.  Over a few
hundred synthetic sets, both phases and ample, tight and insufficient room it proves that every read is listed exactly
once in its class, that the lists are ordered, that slab w holds every store at list position >= w, that slabs neither
overlap nor leave the bytes reported, and that the grids respect their limits.  The giant threshold is set low, as in
the emulated tests, so that the giants' class occurs.
"""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def test_final_stage_slab_planner_on_the_host(tmp_path):
    hipcc = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'
    if not os.path.exists(hipcc):
        pytest.skip('hipcc not available')
    exe = str(tmp_path / 'finplan_check')
    subprocess.check_call([hipcc, '-x', 'c++', '-O1', '-std=c++17', '-w', '-I', os.path.join(HERE, 'native', 'emu'),
                           '-I', os.path.join(HERE, '..', 'include'), '-DBRX_GIANT_UNITS=1048576ull',
                           os.path.join(HERE, 'native', 'finplan_check.hip'), '-o', exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith('ok'), r.stdout[-2000:] + r.stderr[-2000:]
