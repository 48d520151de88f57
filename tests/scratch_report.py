"""The compiler's resource report of one kernel source, for the no-scratch tests: the source is cross-compiled for gfx950 with the
Makefile's flags (`-Rpass-analysis=kernel-resource-usage`) and the report's ScratchSize is read per kernel instance.  No GPU needed."""
import os
import re
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, 'factor-graph-neural-network_amd', 'csrc')
HIPCC = shutil.which('hipcc') or '/opt/rocm/bin/hipcc'


def scratch(src, extra_flags=()):
    """{mangled kernel name: scratch bytes per lane} of csrc/``src``; ``extra_flags``: what the Makefile adds for that source."""
    cmd = [HIPCC, '--offload-arch=gfx950', '-O3', '-std=c++17',      # (the Makefile's flags)
           '-I' + os.path.join(ROOT, 'include'), '-I' + CSRC, '-Wno-unused-function',
           '-Wno-pass-failed', '-fPIC', *extra_flags, '-c', '--cuda-device-only', os.path.join(CSRC, src), '-o', os.devnull,
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
