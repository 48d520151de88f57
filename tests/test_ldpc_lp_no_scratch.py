"""The ADMM-LP decoder kernel keeps a check's state (its w, x[var], old z and row-table words, 16 each, and the cut search over them)
in registers: the compiler's resource report (tests/scratch_report.py) for csrc/ldpc_lp.hip, cross-compiled for gfx950 with the
Makefile's flags for it, shows no scratch for its one kernel instance.  No GPU needed."""
import os

import pytest

from scratch_report import HIPCC, scratch


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_lp_kernel_has_no_scratch():
    rep = scratch('ldpc_lp.hip', ['-ffp-contract=off'])
    print(rep)
    assert len(rep) == 1 and all('ldpc_lp_kernel' in k for k in rep), rep
    assert not any(rep.values()), rep
