"""The LLR-domain LDPC decoders keep a check's whole update in registers: the compiler's resource report
(`-Rpass-analysis=kernel-resource-usage`: ScratchSize) for csrc/ldpc_llr.hip, cross-compiled for gfx950, shows no scratch for any of
the six kernel instances (three algorithms x two schedules) — the sum-product's 16 tanh values and prefix products included.  No GPU
needed.  (The helper is tests/test_no_scratch.py's, with this source's own build flag.)"""
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
def test_llr_decoder_kernels_have_no_scratch():
    rep = _scratch('ldpc_llr.hip')
    hits = {k: v for k, v in rep.items() if 'ldpc_llr_kernel' in k}
    print(hits)
    assert len(hits) == 6, rep                                       # 3 algorithms x 2 schedules
    assert len(rep) == len(hits), rep                                # every kernel instance in the source
    assert not any(hits.values()), hits
