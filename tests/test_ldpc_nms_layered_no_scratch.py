"""The layered learned min-sum kernels keep a check's whole update, forward and backward, in registers: the compiler's resource
report (tests/scratch_report.py) for csrc/ldpc_nms_layered.hip, cross-compiled for gfx950 with the Makefile's flags for it, shows
exactly four kernel instances and no scratch for any of them.  No GPU needed."""
import os

import pytest

from scratch_report import HIPCC, scratch

FAMILIES = {'ldpc_nms_layered_fwd_kernel': 2,       # decode mode, train mode
            'ldpc_nms_layered_bwd_kernel': 2}       # the partial in LDS, in the workspace


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_layered_kernels_have_no_scratch():
    rep = scratch('ldpc_nms_layered.hip', ['-ffp-contract=off'])
    print(rep)
    for family, instances in FAMILIES.items():
        assert sum(family in k for k in rep) == instances, rep
    assert len(rep) == 4, rep                       # the sum of the partials stays ldpc_nms.hip's kernel
    assert not any(rep.values()), rep
