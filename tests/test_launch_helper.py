"""The library launches its kernels in one place, csrc/fgnn_launch.h: a status function that turns a HIP error into
FGNN_ELAUNCH plus "<what> launch: <HIP's text>", a typed and an untyped launcher on top of it, and the one rule for dynamic LDS above
48 KiB.  tests/launch_helper_main.hip checks the status function on fixed codes and the typed launcher on an empty kernel (with a device
both launches succeed, without one both fail with HIP's "no device" text: the program decides); the second test keeps hand-written
launches out of csrc/.  No GPU needed."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'factor-graph-neural-network_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'

# what only fgnn_launch.h may say
LAUNCH_WORDS = ('hipLaunchKernelGGL', 'hipLaunchKernel(', 'hipGetLastError', 'hipFuncSetAttribute')


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_status_function_and_typed_launcher(tmp_path):
    prog = str(tmp_path / 'launch_helper')
    cmd = [HIPCC, '--offload-arch=gfx950', '-O1', '-std=c++17', '-I' + os.path.join(ROOT, 'include'), '-I' + CSRC, '-Wall',
           '-Wno-unused-function', os.path.join(ROOT, 'tests', 'launch_helper_main.hip'), os.path.join(CSRC, 'fgnn_api.hip'), '-o', prog]
    build = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert build.returncode == 0, build.stderr
    run = subprocess.run([prog], capture_output=True, text=True, timeout=120)
    print(run.stdout)
    assert run.returncode == 0, run.stdout + run.stderr
    assert '0 failure(s)' in run.stdout


def test_no_hand_written_launch_in_csrc():
    bad = []
    for name in sorted(os.listdir(CSRC)):
        if name == 'fgnn_launch.h' or not name.endswith(('.hip', '.h')):
            continue
        with open(os.path.join(CSRC, name)) as f:
            for no, line in enumerate(f, 1):
                bad += ['%s:%d: %s' % (name, no, w) for w in LAUNCH_WORDS if w in line]
    assert not bad, 'launch through csrc/fgnn_launch.h instead:\n' + '\n'.join(bad)
