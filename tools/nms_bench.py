#!/usr/bin/env python3
"""The learned min-sum decoder's training path, milliseconds: the forward (train mode: totals and the record), the backward (both
launches) and a whole training step (sampler, LLRs, forward, multi-loss, backward, Adam; replayed as a hipGraph and eagerly), for one
code, batch size, iteration count, sharing mode and schedule.  csrc/ldpc_nms.hip, csrc/ldpc_nms_layered.hip; fgnn_amd/ldpc_nms.py,
ldpc_nms_train.py.

Forward and backward: two warm-up calls, one timed call to size the window (at least 0.2 s of back-to-back calls), then 7 windows
between device events; the median window gives the time (tools/dbench.py's procedure).  The step: ``ldpc_nms_train.train``'s own
clock around its step loop (it ends in a device synchronise), over --steps steps after a run of 20 that warms everything up.
Under ``rocprofv3 --kernel-trace --stats`` (a run of its own; --trace_steps N then runs N eager steps and nothing else) the kernels
are ldpc_nms_fwd_kernel<1>, ldpc_nms_bwd_kernel<..> and ldpc_nms_sum_kernel (layered: ldpc_nms_layered_fwd_kernel<1>,
ldpc_nms_layered_bwd_kernel<..> and the same sum kernel).

    python tools/nms_bench.py [--code builtin] [--words 4096] [--n_iter 5] [--share edge] [--schedule flooding] [--steps 200]
"""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'factor-graph-neural-network_amd'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import torch
from dbench import measure
from fgnn_amd import _hip, ldpc_nms_train
from fgnn_amd.datapath import LdpcDataPath
from fgnn_amd.ldpc_code import LdpcCode
from fgnn_amd.ldpc_nms import SCHEDULES, SHARES, LearnedMinSum, nms_backward_raw, nms_forward_raw


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--code', default='builtin')
    ap.add_argument('--words', type=int, default=4096)
    ap.add_argument('--n_iter', type=int, default=5)
    ap.add_argument('--share', choices=tuple(SHARES), default='edge')
    ap.add_argument('--schedule', choices=SCHEDULES, default='flooding')
    ap.add_argument('--snr', type=float, default=2.0)
    ap.add_argument('--steps', type=int, default=200)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--trace_steps', type=int, default=0, help='run this many eager training steps and nothing else (for a profiler)')
    args = ap.parse_args()
    code = LdpcCode.from_spec(args.code)
    kw = dict(batch_size=args.words, snr=args.snr, n_iter=args.n_iter, share=args.share, code=code, log_every=0, n_epochs=1, schedule=args.schedule)
    with tempfile.TemporaryDirectory() as tmp:
        if args.trace_steps:
            ldpc_nms_train.train(steps_per_epoch=args.trace_steps, graph=False, out_dir=tmp, **kw)
            return
        dev = torch.device('cuda:0')
        path, dec = LdpcDataPath(dev, code), LearnedMinSum(code, args.n_iter, args.share, schedule=args.schedule).to(dev)
        drawn = path.sample_rng(args.words, seed=0, step=0, snr_db=args.snr)
        llr = path.bit_llr(drawn.y, drawn.snr_db)
        tables, sizes, share = (dec.col_ptr, dec.row_ptr, dec.row_edge, dec.row_var), (dec.N, dec.M, dec.E), SHARES[args.share]
        alpha, beta = dec.alpha.detach(), dec.beta.detach()
        layers, lds = dec.layer_tables(), 'fgnn_ldpc_nms_lds_bytes' if args.schedule == 'flooding' else 'fgnn_ldpc_nms_layered_lds_bytes'
        totals, record = nms_forward_raw(llr, tables, sizes, alpha, beta, args.n_iter, share, layers)
        g = torch.randn_like(totals)
        print('# %r, B = %d, n_iter = %d, share = %s, %s: LDS %d B forward, %d B backward state, record %d B per word, workspace %d B' % (
            code, args.words, args.n_iter, args.share, args.schedule, _hip.invoke(lds, *sizes, 0), _hip.invoke(lds, *sizes, 1),
            record.numel() // args.words,
            _hip.invoke('fgnn_ldpc_nms_backward_workspace_bytes', args.words, *sizes, args.n_iter, share)))
        print('%-28s %10s %10s' % ('', 'ms', 'spread %'))
        for label, run in (('forward (train mode)', lambda: nms_forward_raw(llr, tables, sizes, alpha, beta, args.n_iter, share, layers)),
                           ('backward', lambda: nms_backward_raw(g, llr, tables, sizes, alpha, beta, record, args.n_iter, share, layers=layers))):
            med, lo, hi, _ = measure(run, args.repeats)
            print('%-28s %10.4f %10.1f' % (label, med * 1e3, 100 * (hi - lo) / med))
        for graph in (True, False):
            ldpc_nms_train.train(steps_per_epoch=20, graph=graph, out_dir=tmp, **kw)
            r = ldpc_nms_train.train(steps_per_epoch=args.steps, graph=graph, out_dir=tmp, **kw)
            print('%-28s %10.4f %10s   (%d steps, graphed = %s)' % ('training step, ' + ('hipGraph' if graph else 'eager'),
                                                                  1e3 * r['seconds'] / r['steps'], '', r['steps'], r['graphed']))


if __name__ == '__main__':
    main()
