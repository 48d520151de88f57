"""No kernel on the benched LDPC paths may spill: a spill reload is a memory operation whose wait also waits for every load issued before
it — in kernels that keep the next tile / sample in flight that was an HBM round trip per tile.  The check is the
compiler's own resource report (`-Rpass-analysis=kernel-resource-usage`: ScratchSize) for the sources of those kernels, cross-compiled for
gfx950 — no GPU needed."""
import os
from concurrent.futures import ThreadPoolExecutor

import pytest

from scratch_report import HIPCC, scratch

# source -> the kernels (mangled-name substrings) that must have no scratch; other instances in the same source are reported, not asserted
MUST = {
    'factor_layer_fwd.hip': ['factor_layer_fwd_kernel'],
    'mpconv_block_fwd.hip': ['mpconv_block_fwd_kernel', 'mpconv_block_rows1_kernel', 'mpconv_block_fanin_kernel', 'mpconv_block_fanout_kernel'],
    'linear_fwd_b16.hip': ['linear_fwd_b16_kernel', 'linear_instnorm_fwd_kernel', 'linear_multi_b16_kernel'],
    'mpconv_bwd_ws.hip': ['mpconv_bwd_ws_kernel'],
    'block_tail.hip': ['block_tail_kernel', 'block_head_bwd_kernel'],
    'mpconv_fwd_ws.hip': ['mpconv_fwd_ws_kernelILi64E'],          # (the 128-input instances spill at their 128-register budget: consumers only, profiles/r06/README.md)
}
FLAGS = {'block_tail.hip': ('-fno-slp-vectorize',)}          # what the Makefile adds per source


@pytest.mark.skipif(not os.path.exists(HIPCC), reason='no hipcc')
def test_benched_kernels_have_no_scratch():
    with ThreadPoolExecutor(max_workers=len(MUST)) as ex:
        reports = dict(zip(MUST, ex.map(lambda src: scratch(src, FLAGS.get(src, ())), MUST)))
    bad = []
    for src, subs in MUST.items():
        rep = reports[src]
        assert rep, 'no resource report for %s' % src
        for sub in subs:
            hits = {k: v for k, v in rep.items() if sub in k}
            assert hits, (src, sub)
            bad += ['%s: %s spills %d bytes per lane' % (src, k, v) for k, v in hits.items() if v]
    assert not bad, '\n'.join(bad)
