"""The learned min-sum decoder keeps a check's update in registers, forward and backward: the compiler's resource report
(`-Rpass-analysis=kernel-resource-usage`: ScratchSize) for csrc/ldpc_nms.hip, cross-compiled for gfx950, shows no scratch for any of
its five kernel instances (the forward's decode and train modes, the backward with its partial in LDS and in the workspace, the sum
of the partials).  No GPU needed.  (The helper is tests/test_ldpc_llr_no_scratch.py's, restated.)"""
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'factor-graph-neural-network_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


def _scratch(src):
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17',      # (the Makefile's flags)
           '-I' + os.path.join(ROOT, 'include'), '-I' + CSRC, '-Wno-unused-function',
           '-Wno-pass-failed', '-fPIC', '-ffp-contract=off', '-c', '--cuda-device-only', os.path.join(CSRC, src), '-o', os.devnull,
           '-Rpass-analysis=kernel-resource-usage']
    err = subprocess.run(cmd, capture_output=True, text=True, timeout=1500).stderr
    out, name = {}, None
    for line in err.splitlines():
        m = re.search(r'Function Name: (\S+)', line)
        if m:
            name = m.group(1)
        m = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', line)
        if m and name:
            out[name] = int(m.group(1))
    return out


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_learned_min_sum_kernels_have_no_scratch():
    rep = _scratch('ldpc_nms.hip')
    print(rep)
    hits = {k: v for k, v in rep.items() if 'ldpc_nms_' in k}
    assert sum('ldpc_nms_fwd_kernel' in k for k in hits) == 2, rep      # decode mode, train mode
    assert sum('ldpc_nms_bwd_kernel' in k for k in hits) == 2, rep      # the partial in LDS, in the workspace
    assert sum('ldpc_nms_sum_kernel' in k for k in hits) == 1, rep
    assert len(rep) == len(hits) == 5, rep                              # every kernel instance in the source
    assert not any(hits.values()), hits
