"""The LDPC decoder kernels keep their per-thread state in registers: the compiler's resource report (tests/scratch_report.py) for
each source, cross-compiled for gfx950 with the Makefile's flags for it, shows no scratch for any kernel instance.  No GPU needed.

  * csrc/ldpc_llr.hip: a check's whole update, the sum-product's 16 tanh values and prefix products included;
  * csrc/ldpc_nms.hip: a check's update, forward and backward;
  * csrc/ldpc_osd.hip: the ranks a thread counts and its rows' flags."""
import os

import pytest

from scratch_report import HIPCC, scratch

SOURCES = {     # source: (the Makefile's flags for it, {kernel family: its instances})
    'ldpc_llr.hip': (['-ffp-contract=off'], {'ldpc_llr_kernel': 6}),                    # 3 algorithms x 2 schedules
    'ldpc_nms.hip': (['-ffp-contract=off'], {'ldpc_nms_fwd_kernel': 2,                  # decode mode, train mode
                                             'ldpc_nms_bwd_kernel': 2,                  # the partial in LDS, in the workspace
                                             'ldpc_nms_sum_kernel': 1}),                # the sum of the partials
    'ldpc_osd.hip': ([], {'ldpc_osd_kernel': 1}),                                       # the one kernel
}


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
@pytest.mark.parametrize('src', SOURCES)
def test_decoder_kernels_have_no_scratch(src):
    flags, families = SOURCES[src]
    rep = scratch(src, flags)
    print(rep)
    for family, instances in families.items():
        assert sum(family in k for k in rep) == instances, rep
    assert len(rep) == sum(families.values()), rep                   # every kernel instance in the source belongs to one family
    assert not any(rep.values()), rep
