"""Training learned min-sum LDPC decoders (``ldpc_nms.LearnedMinSum``) on the GPU, from sampling to the checkpoint.

The reference has no such decoder; the loop is ``ldpc_train``'s over the same pieces (``trainloop``): every batch is drawn on the device
in one launch (``LdpcDataPath.sample_rng(batch_size, seed, step=gcnt, snr_db=snr)``, written into the buffers the captured step reads),
the decoder runs on the channel LLRs ``bit_llr(y, snr_db)``, the loss is ``ldpc_nms.multi_loss`` against the transmitted codeword,
forward / loss / backward are replayed as one hipGraph, Adam is the one-kernel ``FastAdam`` and the host reads nothing back between log
lines.  Unlike ``ldpc_train`` it takes every code the LLR-domain decoders take (``LdpcCode.require_llr_decoder``: N, M <= 1024, degrees
<= 16), e.g. ``--code gallager:1024,4,8,2``.

    python -m fgnn_amd.ldpc_nms_train --code gallager:384,3,6,1 --n_iter 10 --out_dir ckpt
    python -m fgnn_amd.ldpc_eval --curve --code gallager:384,3,6,1 --decoder learned-min-sum:ckpt/LearnedMinSum_edge_10_epoches_10_snr_None.pt
"""
import argparse
import os
import sys
import time

import torch

from . import trainloop
from .ldpc_train import default_steps_per_epoch

LR = 1e-2
SAVE_EVERY = 10
LOG_EVERY = 10


def lr_sched(epoch):
    """The ``LambdaLR`` factor: the rate stays ``lr`` (a few hundred parameters near their optimum from the start need no warm-up)."""
    return 1.0


def checkpoint_dict(model, optimizer, scheduler, epoch, gcnt):
    """``ldpc_train``'s dict plus 'decoder' (kind, n_iter, share and, where it is not flooding, schedule: what
    ``ldpc_nms.load_checkpoint`` rebuilds the module from); for a non-default code only, plus its 'code' entry (``LdpcCode.checkpoint_entry``), by
    which a reader refuses another code's decoder."""
    d = {'model_state_dict': model.state_dict(), 'optimizer_state_dict': optimizer.state_dict(), 'lr_sche': scheduler.state_dict(),
         'epoch': int(epoch), 'gcnt': int(gcnt), 'decoder': model.decoder_entry()}
    if not model.code.is_default:
        d['code'] = model.code.checkpoint_entry()
    return d


def checkpoint_path(out_dir, model_name, model, epoch, snr):
    """``MODEL_SHARE_NITER_epoches_EPOCH_snr_SNR.pt``; a layered decoder's has ``layered_`` before the iteration count."""
    sched = '' if model.schedule == 'flooding' else model.schedule + '_'
    return os.path.join(out_dir, '{}_{}_{}{}_epoches_{}_snr_{}.pt'.format(model_name, model.share, sched, model.n_iter, epoch, snr))


def train(n_epochs=10, batch_size=256, snr=None, n_iter=5, share='edge', model_path=None, model_name='LearnedMinSum', steps_per_epoch=None,
          seed=0, out_dir='.', save_every=SAVE_EVERY, log_every=LOG_EVERY, graph=True, test_set=None, lr=LR, device='cuda', code=None,
          alpha=0.8125, beta=0.0, schedule='flooding'):
    """Train ``LearnedMinSum(code, n_iter, share, alpha, beta, schedule)`` for ``n_epochs`` epochs of ``steps_per_epoch`` batches (default:
    ``ldpc_train``'s ceil(10000 / batch_size)).  ``code``: an ``LdpcCode`` within ``require_llr_decoder``'s limits (None: the built-in
    96.3.963; ValueError otherwise, before anything reaches the device).  Batch number ``gcnt`` (counted from 0 over the whole run,
    resumes included) is ``sample_rng(batch_size, seed, step=gcnt, snr_db=snr)``: SNR drawn from {0..4} dB per word unless ``snr`` fixes
    it, bursts as the sampler draws them; the decoder sees ``bit_llr(y, snr_db)``.  Loss: ``multi_loss(totals, cw)``.  Optimizer:
    ``FastAdam(lr)``; ``LambdaLR(lr_sched)`` is stepped at the end of every epoch.

    ``graph``: zero_grad, LLRs, forward, loss and backward are captured once (``graph.StepGraph``) and replayed; the sampler launch and
    ``opt.step()`` run eagerly around the replay.  A failed capture prints one line on stderr and the run goes on with eager steps.
    Each step's loss goes into a device ring and the decision counts of the last iteration's totals accumulate on the device; whenever
    ``gcnt`` reaches a multiple of ``log_every`` they are read and a line ``epoch = .. bcnt = .. loss = .. acc = ..`` is printed (means
    over the steps since the previous line; ``acc``: the fraction of the N bits decided as sent).  0 / None: no lines, one read every
    256 steps.

    Checkpoints (``checkpoint_dict``) go to ``checkpoint_path(...)``: at the top of an epoch when ``(epoch + 1) % save_every == 0`` and
    after the last epoch with ``epoch = n_epochs``.  ``model_path`` resumes from one (its n_iter, share and schedule must be the arguments').
    ``test_set`` (a path or a dict, ``ldpc_eval.load_test_set``): after the last epoch the decoder's decode mode runs on it and the
    ``ber`` / ``err_class`` of ``ldpc_eval.LdpcErrorCounts`` over the K message bits are printed and returned.

    Returns a dict: loss and acc of the last log window, losses (every step's, f32 values), steps, gcnt, seconds (the step loops only),
    graphed, checkpoint (the last one's path), and ber / err_class when evaluated."""
    from .ldpc_code import LdpcCode
    from .ldpc_nms import LearnedMinSum, multi_loss
    code = LdpcCode.builtin() if code is None else code
    code.require_llr_decoder()
    n_epochs, batch_size, seed = int(n_epochs), int(batch_size), int(seed)
    steps_per_epoch = default_steps_per_epoch(batch_size) if steps_per_epoch is None else int(steps_per_epoch)
    save_every = int(save_every)
    if n_epochs < 0 or batch_size < 1 or steps_per_epoch < 1 or save_every < 1:
        raise ValueError('n_epochs >= 0, batch_size >= 1, steps_per_epoch >= 1 and save_every >= 1 needed')
    model = LearnedMinSum(code, n_iter, share, alpha, beta, schedule)
    dev = trainloop.cuda_device(device)
    from .datapath import LdpcDataPath
    from .fastpath import FastAdam

    ckpt = None
    if model_path:
        ckpt = torch.load(model_path, map_location='cpu', weights_only=True)
        if ckpt.get('decoder') != model.decoder_entry():
            raise ValueError('%s holds %r, not %r' % (model_path, ckpt.get('decoder'), model.decoder_entry()))
        code.check_checkpoint(ckpt, model_path)
        model.load_state_dict(ckpt['model_state_dict'], strict=True)
    model.to(dev).train()
    opt = FastAdam(model.parameters(), lr=lr)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lr_sched)
    start_epoch, gcnt = (0, 0) if ckpt is None else trainloop.resume(ckpt, opt, sched)
    path = LdpcDataPath(dev, code)
    static = path.sample_rng(batch_size, seed, step=gcnt, snr_db=snr)                   # the buffers every step reads
    draw = lambda step: path.sample_rng(batch_size, seed, step=step, snr_db=snr, out=static)

    window = trainloop.LogWindow(dev, 1, 2, log_every)       # rows {loss}; counts {bits, bits decided as sent}
    keep = {}

    def compute():
        opt.zero_grad()
        totals = model(path.bit_llr(static.y, static.snr_db))
        loss = multi_loss(totals, static.cw)
        loss.backward()
        with torch.no_grad():
            window.counts[0] += static.cw.numel()
            window.counts[1] += ((totals[-1] < 0) == (static.cw != 0)).sum()
        keep['row'] = loss.detach().reshape(1)

    graphed = None
    if graph and start_epoch < n_epochs:
        graphed = trainloop.capture_step(compute, [model], window.counts, 'ldpc_nms_train')

    last = {'loss': None, 'acc': None}

    def drain(epoch, bcnt, say):
        """Read the window back (its one synchronisation) and start the next one."""
        read = window.read()
        if read is None:
            return
        got, (n, right) = read
        last.update(loss=sum(row[0] for row in got) / len(got), acc=right / n if n else None)
        if say:
            print('epoch = {} bcnt = {} loss = {} acc = {}'.format(epoch, bcnt, last['loss'], last['acc']), flush=True)

    os.makedirs(out_dir, exist_ok=True)
    saved_to = None

    def save(epoch):
        nonlocal saved_to
        saved_to = checkpoint_path(out_dir, model_name, model, epoch, snr)
        torch.save(checkpoint_dict(model, opt, sched, epoch, gcnt), saved_to)

    seconds, steps = 0.0, 0
    for epoch in range(start_epoch, n_epochs):
        if (epoch + 1) % save_every == 0:
            save(epoch)
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for bcnt in range(steps_per_epoch):
            draw(gcnt)
            if graphed is not None:
                graphed.replay()
            else:
                compute()
            full = window.push(keep['row'])
            opt.step()
            gcnt += 1
            steps += 1
            if (log_every and gcnt % log_every == 0) or full:
                drain(epoch, bcnt, bool(log_every))
        torch.cuda.synchronize(dev)
        seconds += time.perf_counter() - t0
        sched.step()
    drain(n_epochs - 1, steps_per_epoch - 1, False)      # the steps behind the last line: a last, shorter window
    if start_epoch < n_epochs:
        save(n_epochs)
    result = {'model_name': model_name, 'loss': last['loss'], 'acc': last['acc'], 'losses': window.losses, 'steps': steps, 'gcnt': gcnt,
              'seconds': seconds, 'graphed': graphed is not None, 'checkpoint': saved_to}
    if test_set is not None:
        from .ldpc_eval import LdpcErrorCounts, load_test_set
        y, gts, snr_t, sb = load_test_set(test_set, dev, code.n_var)
        acc = LdpcErrorCounts(dev)
        for i in range(0, y.shape[0], 4096):
            rows = slice(i, min(y.shape[0], i + 4096))
            snr0 = snr_t[rows] if snr_t.dim() == 1 else snr_t[rows, 0]
            acc.add_bits(model.decode(path.bit_llr(y[rows], snr0))[0], gts[rows], snr_t[rows], sb[rows], nbits=code.K)
        res = acc.result()
        result.update(ber=res['ber'], err_class=res['err_class'])
        print(res['ber'])
        print(torch.FloatTensor(res['err_class']))
    return result


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m fgnn_amd.ldpc_nms_train',
                                 description='Train a learned min-sum LDPC decoder on batches drawn on the GPU and write its checkpoints '
                                             '(python -m fgnn_amd.ldpc_eval --decoder learned-min-sum:CHECKPOINT reads them).')
    ap.add_argument('--n_epochs', type=int, default=10)
    ap.add_argument('--batch_size', type=int, default=256)
    ap.add_argument('--snr', type=int, default=None, help='one SNR (dB) for every word; default: 0..4 dB per word')
    ap.add_argument('--n_iter', type=int, default=5, help='decoding iterations (1..64), each with weights of its own')
    ap.add_argument('--share', choices=('iteration', 'check', 'edge'), default='edge', help='one alpha / beta per iteration, per check or per edge')
    ap.add_argument('--schedule', choices=('flooding', 'layered'), default='flooding',
                    help='flooding, or layered: the checks layer by layer, each on the totals the earlier layers left')
    ap.add_argument('--lr', type=float, default=LR)
    ap.add_argument('--model_path', default=None, help='resume from this checkpoint')
    ap.add_argument('--model_name', default='LearnedMinSum')
    ap.add_argument('--steps_per_epoch', type=int, default=None, help='default: ceil(10000 / batch_size)')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out_dir', default='.', help='where the checkpoints go')
    ap.add_argument('--save_every', type=int, default=SAVE_EVERY)
    ap.add_argument('--log_every', type=int, default=LOG_EVERY)
    ap.add_argument('--no-graph', dest='graph', action='store_false', help='eager steps, no hipGraph replay')
    ap.add_argument('--test_path', default=None, help='test set to evaluate on after the last epoch (ldpc_eval)')
    ap.add_argument('--code', default='builtin', help='builtin (96.3.963), the path of an alist file, or gallager:N,dv,dc,seed (N, M <= 1024, degrees <= 16)')
    ap.add_argument('--json', action='store_true', help='print the result as one JSON line at the end')
    args = ap.parse_args(argv)
    from .ldpc_code import LdpcCode
    r = train(args.n_epochs, args.batch_size, args.snr, args.n_iter, args.share, trainloop.existing_or_none(args.model_path),
              args.model_name, args.steps_per_epoch, args.seed, args.out_dir, args.save_every, args.log_every, args.graph, args.test_path,
              args.lr, 'cuda:0', LdpcCode.from_spec(args.code), schedule=args.schedule)
    if 'err_class' in r:                 # (an array: as lists for the JSON line; the last key either way)
        r['err_class'] = [[float(v) for v in row] for row in r['err_class']]
    trainloop.report(r, args.json)
    return 0


if __name__ == '__main__':
    sys.exit(main())
