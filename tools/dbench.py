#!/usr/bin/env python3
"""Classical LDPC decoders, words per second: the f64 probability-domain decoder (LdpcDataPath.decode, 100 loops: csrc/ldpc_decode.hip)
against the LLR-domain decoders (LdpcDataPath.decode_llr, max_iter 50: csrc/ldpc_llr.hip), every algorithm x schedule.

4096 received words of the all-zero codeword at 2 dB (no burst; one fixed torch seed), for the built-in 96.3.963 and for
gallager(384, 3, 6, 1) and gallager(1024, 4, 8, 2) (which the f64 decoder refuses).  Per decoder: two warm-up calls, one timed call
to size the window (at least 0.2 s of back-to-back calls), then 7 windows between device events; the median window gives the rate.  Also printed: mean iterations
and the decoded fraction (words that end with no violated check), and the LDS bytes a word occupies.

The learned min-sum decoder (fgnn_amd.ldpc_nms.LearnedMinSum.decode, csrc/ldpc_nms.hip: the decode mode, early stopping) follows,
beside min-sum:flooding at the same iteration count (--learned_iters), with untrained weights (alpha 0.8125, beta 0: the same
decisions) shared per iteration, per check and per edge: the weight reads are its only extra work in the loop.  Its layered schedule
(schedule='layered', csrc/ldpc_nms_layered.hip; rows ``learned layered ...``) follows in the same way beside min-sum:layered at that iteration count.

Ordered-statistics reprocessing (LdpcDataPath.decode_osd, csrc/ldpc_osd.hip) follows as min-sum:layered:osd=0|1|2 (order 2: the
default span, 64), each row the whole composition ``ldpc_decoders.Decoder.run`` runs — the decoder with posteriors, then the reprocessing
of the words it leaves with violated checks — to be read beside the plain min-sum:layered row; ``decoded`` is 1 there by construction.
A third code, gallager(384, 3, 6, 1), sits between the two (128 threads per word).

The ADMM linear-programming decoder (LdpcDataPath.decode_lp, csrc/ldpc_lp.hip) closes each code's rows as ``admm-lp`` (the plain LP:
max_iter 200, stopped by its residual rule; one more column, the fraction of words that carry the ML certificate) and
``admm-lp:penalty=0.8`` (the penalised decoder, stopped on a codeword), to be read beside the min-sum and sum-product rows.

    python tools/dbench.py [--words 4096] [--snr 2.0] [--repeats 7] [--learned_iters 5]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'factor-graph-neural-network_amd'))
import torch
from fgnn_amd import _hip
from fgnn_amd.datapath import LdpcDataPath
from fgnn_amd.ldpc_code import LdpcCode
from fgnn_amd.ldpc_decoders import LLR_ALGORITHMS, LLR_SCHEDULES, parse_decoder
from fgnn_amd.ldpc_nms import SHARES, LearnedMinSum


def window(run, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        out = run()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1e-3, out


def measure(run, repeats):
    """Seconds per call (median of ``repeats`` windows, lowest, highest) and the last call's result."""
    for _ in range(2):
        run()
    torch.cuda.synchronize()
    once, _ = window(run, 1)
    calls = max(1, min(1000, int(0.2 / max(once, 1e-6)) + 1))
    times = []
    for _ in range(repeats):
        t, out = window(run, calls)
        times.append(t / calls)
    return statistics.median(times), min(times), max(times), out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('--words', type=int, default=4096)
    ap.add_argument('--snr', type=float, default=2.0)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--learned_iters', type=int, default=5)
    args = ap.parse_args()
    dev = torch.device('cuda:0')
    print('%-24s %-34s %12s %10s %10s %9s %9s' % ('code', 'decoder', 'words/s', 'us/call', 'spread %', 'iters', 'decoded'))
    for name, code in (('builtin 96.3.963', LdpcCode.builtin()), ('gallager(384,3,6,1)', LdpcCode.gallager(384, 3, 6, 1)),
                       ('gallager(1024,4,8,2)', LdpcCode.gallager(1024, 4, 8, 2))):
        path = LdpcDataPath(dev, code)
        gen = torch.Generator(device=dev).manual_seed(0)
        gcx = 10.0 ** (args.snr / 20.0)
        y = -gcx + torch.randn((args.words, code.n_var), device=dev, generator=gen)
        snr = torch.full((args.words,), args.snr, device=dev)
        llr, bias = path.bit_llr(y, snr), path.bit_prior(y, snr)
        E = code.n_var * code.dv
        print('# %s: %s, %d LDS bytes per word for decode_llr, %d for decode_osd'
              % (name, code, _hip.invoke('fgnn_ldpc_decode_llr_lds_bytes', code.n_var, code.n_chk, E),
                 _hip.invoke('fgnn_ldpc_osd_lds_bytes', code.n_var, code.n_chk)))
        runs = []
        try:
            code.require_decoder()
            runs.append(('mackay f64 (100 loops)', lambda: path.decode(bias, loops=100)))
        except ValueError as e:
            print('%-24s %-34s refused: %s' % (name, 'mackay f64 (100 loops)', e))
        for alg in LLR_ALGORITHMS:
            for sched in LLR_SCHEDULES:
                runs.append(('%s:%s' % (alg, sched), lambda alg=alg, sched=sched: path.decode_llr(llr, alg, sched, max_iter=50)))
        for order in (0, 1, 2):
            decoder = parse_decoder('min-sum:layered:osd=%d' % order)
            runs.append((decoder.spec, lambda decoder=decoder: decoder.run(path, y, snr)))
        n = args.learned_iters
        runs.append(('min-sum:flooding:iters=%d' % n, lambda: path.decode_llr(llr, 'min-sum', 'flooding', max_iter=n)))
        for share in SHARES:
            dec = LearnedMinSum(code, n, share).to(dev)
            runs.append(('learned-min-sum %s iters=%d' % (share, n), lambda dec=dec: dec.decode(llr)))
        runs.append(('min-sum:layered:iters=%d' % n, lambda: path.decode_llr(llr, 'min-sum', 'layered', max_iter=n)))
        for share in SHARES:
            dec = LearnedMinSum(code, n, share, schedule='layered').to(dev)
            runs.append(('learned layered %s iters=%d' % (share, n), lambda dec=dec: dec.decode(llr)))
        lp_bytes = _hip.invoke('fgnn_ldpc_decode_lp_lds_bytes', code.n_var, code.n_chk, E)
        print('# %s: %d LDS bytes per word for decode_lp' % (name, lp_bytes))
        for spec in ('admm-lp', 'admm-lp:penalty=0.8'):
            if lp_bytes >= 0:
                runs.append((spec, lambda kw=parse_decoder(spec).args: path.decode_lp(llr, **kw)))
        for label, run in runs:
            med, lo, hi, (x, viol, iters, *flags) = measure(run, args.repeats)
            # the plain LP's last column: the fraction of words that carry the ML certificate (flag bit 1)
            certified = '   certified %.4f' % (flags[0] & 2 != 0).float().mean().item() if label == 'admm-lp' else ''
            print('%-24s %-34s %12.0f %10.1f %10.1f %9.2f %9.4f%s' % (name, label, args.words / med, med * 1e6, 100 * (hi - lo) / med,
                                                                     iters.float().mean().item(), (viol == 0).float().mean().item(), certified))


if __name__ == '__main__':
    main()
