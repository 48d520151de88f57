"""The bf16 instances of the hyper-factor fan-in backward kernel (csrc/mpconv_bwd_hyper.hip::mpconv_bwd_fanin_kernel) keep their
weight-gradient accumulators — 64 or 128 registers per lane — and everything else in registers: no scratch, in the 64->64, 128->64 and
64->128 instances, for the channel-fastest layout and for the element-access one.  The compiler's own resource report, cross-compiled
for gfx950 — no GPU needed."""
import os

import pytest

from scratch_report import HIPCC, scratch

INSTANCES = ['Li1ELi1E', 'Li2ELi1E', 'Li1ELi2E']          # <NI, NO> as the mangled names spell them


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_bf16_fan_in_backward_instances_have_no_scratch():
    rep = scratch('mpconv_bwd_hyper.hip')
    assert rep, 'no resource report for mpconv_bwd_hyper.hip'
    fanin = {k: v for k, v in rep.items() if 'mpconv_bwd_fanin_kernel' in k and '6bf16_t' in k}
    for inst in INSTANCES:
        hits = {k: v for k, v in fanin.items() if inst in k}
        assert hits, (inst, sorted(rep))
        for k, v in hits.items():
            print('%s: ScratchSize %d' % (k, v))
        assert all(v == 0 for v in hits.values()), hits
