"""Training LDPC decoders on the GPU: the loop of the reference's ``train_ldpc.py``, from sampling to the checkpoint.

The reference's loop (/root/reference/train_ldpc.py:150-259) reads ``ContinousCodesSP`` items through a DataLoader (a host encode and
channel per item), runs ``LDPCModel``, takes BCE-with-logits on the 48 message bits plus 0.1 x the MSE of the burst-amplitude
regressor, steps ``Adam(lr=1e-2, weight_decay=1e-8)`` under a warm-up / decay ``LambdaLR`` stepped at the end of every epoch, reads
three numbers back per step for its log line and saves a checkpoint every tenth epoch.  Here every batch is drawn on the device in one
launch (``LdpcDataPath.sample_rng(batch_size, seed, step=gcnt)``, written into the buffers the captured step reads), the loss, its
two terms and the decision counts are one kernel (``decoding_loss_parts``), the forward / loss / backward are replayed as one
hipGraph, Adam is the one-kernel ``FastAdam``, and the host reads nothing back between log lines.  The checkpoints are the script's
dict: ``python -m fgnn_amd.ldpc_eval --model_path`` reads them, and they are laid out for ``train_ldpc.py --model_path``: the model's
keys are the script's class's (tests/test_host_logic.py::test_ldpc_model_state_dict_surface), and a stock ``torch.optim.Adam`` /
``LambdaLR`` composed as the script composes them load the other two dicts (tests/test_ldpc_train.py).

``python -m fgnn_amd.ldpc_train --n_epochs 20 --batch_size 4096`` is the command line; ``--code`` (``train(code=...)``) trains a decoder
for another regular code (``fgnn_amd.ldpc_code.LdpcCode``), which the reference cannot: its checkpoint carries the code it was trained for.
"""
import argparse
import contextlib
import os
import sys
import time

import torch

from . import trainloop

LR = 1e-2                            # train_ldpc.py:160-161
WEIGHT_DECAY = 1e-8
MSE_WEIGHT = 0.1                     # train_ldpc.py:227
TRAIN_SIZE = 10000                   # len(ContinousCodesSP), ldpc_dataset.py: an epoch is ceil(TRAIN_SIZE / batch_size) steps
SAVE_EVERY = 10                      # train_ldpc.py:199
LOG_EVERY = 10                       # train_ldpc.py:242


def lr_sched(x, start=10):
    """The script's ``LambdaLR`` factor (train_ldpc.py:163-167): a linear warm-up from 1e-2 over ``start`` epochs, then 0.99 per epoch."""
    if x <= start:
        return max(1e-2, (1.0 / start) * x)
    return max(0.99 ** (x - start), 1e-6)


def epoch_lr(epoch, lr=LR):
    """The rate 0-based epoch ``epoch`` trains at: the script steps the scheduler at the END of every epoch (train_ldpc.py:253), so
    epoch 0 runs at ``lr * lr_sched(0)`` = 1e-4."""
    return lr * lr_sched(epoch)


def default_steps_per_epoch(batch_size):
    """Batches of a DataLoader over the 10000 items of ``ContinousCodesSP`` (the last one is short there; here every batch is full)."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError('batch_size must be >= 1')
    return -(-TRAIN_SIZE // batch_size)


def checkpoint_dict(model, optimizer, scheduler, epoch, gcnt, code=None):
    """The dict the script saves (``get_model_dict``, train_ldpc.py:185-192); for a non-default ``code`` only, plus a 'code' entry
    (``LdpcCode.checkpoint_entry``: n_var, n_chk, dv, dc and var_to_factors as tensors) by which a reader refuses another code's model."""
    d = {'model_state_dict': model.state_dict(), 'optimizer_state_dict': optimizer.state_dict(), 'lr_sche': scheduler.state_dict(),
         'epoch': int(epoch), 'gcnt': int(gcnt)}
    if code is not None and not code.is_default:
        d['code'] = code.checkpoint_entry()
    return d


def checkpoint_path(out_dir, model_name, epoch, snr):
    """``get_model_path`` (train_ldpc.py:194-195)."""
    return os.path.join(out_dir, '{}_nn_factor_epoches_{}_snr_{}.pt'.format(model_name, epoch, snr))


def _scheduler(opt):
    return torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lr_sched)


def build_model(aggregator='max', code=None):
    """``LDPCModel(2, 6, 4)`` as the script builds it (train_ldpc.py:335), or ``LDPCModel.for_code(code)`` for a non-default code; its
    construction prints, stdout stays the caller's."""
    from .ldpc import LDPCModel
    with contextlib.redirect_stdout(sys.stderr):
        if code is None or code.is_default:
            return LDPCModel(2, 6, 4, aggregator=aggregator)
        return LDPCModel.for_code(code, 4, aggregator=aggregator)


def train(n_epochs=10, batch_size=32, snr=None, aggregator='max', model_path=None, model_name='FactorNN', steps_per_epoch=None,
          dtype=torch.bfloat16, seed=0, out_dir='.', save_every=SAVE_EVERY, log_every=LOG_EVERY, graph=True, test_set=None, lr=LR,
          device='cuda', code=None):
    """``code``: an ``LdpcCode`` (None: the built-in 96.3.963, exactly as before) within ``LdpcCode.require_trainer``'s limits (dv = 3,
    dc = 6, N <= 96; ValueError otherwise, before anything reaches the device): the sampler, the model (``LDPCModel.for_code``), the
    K label bits and the evaluation follow it, and the checkpoints carry a 'code' entry that ``model_path`` and ``ldpc_eval`` check.

    Train ``LDPCModel(2, 6, 4, aggregator)`` for ``n_epochs`` epochs of ``steps_per_epoch`` batches (default: the script's
    ceil(10000 / batch_size)).  Batch number ``gcnt`` (counted from 0 over the whole run, resumes included) is
    ``LdpcDataPath.sample_rng(batch_size, seed, step=gcnt, dtype, snr_db=snr)``: SNR drawn from {0..4} dB per word unless ``snr`` fixes
    it, as ``ContinousCodesSP(snr=args.snr)``; ``make_test_set`` draws at offsets from 2^62, so no test word shares noise with a
    training batch.  Loss ``decoding_loss_parts`` (BCE + 0.1 MSE), optimizer ``FastAdam(model.parameters(), lr, weight_decay=1e-8)``
    over ALL parameters as the script passes them (the frozen tables ride along: ``state_dict()`` numbers parameters as stock Adam
    does), ``LambdaLR(lr_sched)`` stepped at the end of every epoch (epoch e trains at ``epoch_lr(e, lr)``).  Features are in
    ``dtype`` (bf16: the forward runs under bf16 autocast); parameters and Adam state are f32.  ``seed`` also seeds the parameter
    initialisation.

    ``graph``: zero_grad, forward, loss and backward are captured once (``graph.StepGraph``) and replayed; the sampler launch (into
    the captured input buffers) and ``opt.step()`` run eagerly around the replay.  A failed capture prints one line on stderr and the
    run goes on with eager steps, from the buffers and counts ``graph=False`` starts from.  Nothing is read back per step: each step's
    {total, BCE, MSE} goes into a device ring and the decision counts accumulate on the device; whenever ``gcnt`` reaches a multiple of
    ``log_every`` (counted over the whole run, across epochs and resumes, as the script's ``gcnt % 10 == 0``) they are read and the
    script's line ``epoch = .. bcnt = .. loss = .. acc = ..`` is printed with ``sigma_b_loss = ..`` behind it: ``loss`` is the BCE mean,
    as in the script, and the three figures are means over the steps since the previous line (the script also restarts its lists at
    the top of an epoch, so its first line of an epoch averages fewer steps; here a window does not end at an epoch boundary and the
    host does not wait there).  0 / None: no log lines, one read every 256 steps.  The steps behind the last line form a last,
    shorter window, read once at the end.

    Checkpoints (``checkpoint_dict``) go to ``checkpoint_path(out_dir, model_name, epoch, snr)``: at the top of an epoch when
    ``(epoch + 1) % save_every == 0`` and after the last epoch with ``epoch = n_epochs``.  ``model_path`` resumes from one: parameters,
    Adam state, scheduler, epoch and ``gcnt``.  ``test_set`` (a path or a dict, ``ldpc_eval.load_test_set``): after the last epoch
    ``ldpc_eval.evaluate(model, test_set, dtype=dtype)`` runs and its ``ber`` / ``err_class`` are printed and returned.

    Returns a dict: loss (BCE mean), sigma_b_loss and acc of the last log window, losses (every step's total, f32 values), steps, gcnt,
    seconds (the step loops only), graphed, checkpoint (the last one's path), and ber / err_class when evaluated."""
    from .ldpc_code import LdpcCode
    code = LdpcCode.builtin() if code is None else code
    code.require_trainer()
    n_epochs, batch_size, seed = int(n_epochs), int(batch_size), int(seed)
    steps_per_epoch = default_steps_per_epoch(batch_size) if steps_per_epoch is None else int(steps_per_epoch)
    save_every = int(save_every)
    if n_epochs < 0 or batch_size < 1 or steps_per_epoch < 1 or save_every < 1:
        raise ValueError('n_epochs >= 0, batch_size >= 1, steps_per_epoch >= 1 and save_every >= 1 needed')
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError('dtype must be float32 or bfloat16')
    dev = trainloop.cuda_device(device)
    from .datapath import LdpcDataPath
    from .fastpath import FastAdam
    from .ldpc import decoding_loss_parts

    torch.manual_seed(seed)
    model = build_model(aggregator, code)
    ckpt = None
    if model_path:
        ckpt = torch.load(model_path, map_location='cpu', weights_only=True)
        code.check_checkpoint(ckpt, model_path)
        model.load_state_dict(ckpt['model_state_dict'], strict=True)
    model.to(dev).train()
    opt = FastAdam(model.parameters(), lr=lr, weight_decay=WEIGHT_DECAY)
    sched = _scheduler(opt)
    start_epoch, gcnt = (0, 0) if ckpt is None else trainloop.resume(ckpt, opt, sched)
    path = LdpcDataPath(dev, code)
    static = path.sample_rng(batch_size, seed, step=gcnt, dtype=dtype, snr_db=snr)       # the buffers every step reads
    draw = lambda step: path.sample_rng(batch_size, seed, step=step, dtype=dtype, snr_db=snr, out=static)

    window = trainloop.LogWindow(dev, 3, 2, log_every)       # rows {total, BCE, MSE}; counts {bits, bits decided as the label}
    keep = {}
    amp = torch.autocast('cuda', dtype=torch.bfloat16, enabled=dtype == torch.bfloat16)

    def compute():
        opt.zero_grad()
        with amp:
            logits, pred = model(*static[:6])
        loss, parts = decoding_loss_parts(logits, pred, static.label, static.sigma_b, MSE_WEIGHT, window.counts)
        loss.backward()
        keep['parts'] = parts

    graphed = None
    if graph and start_epoch < n_epochs:
        graphed = trainloop.capture_step(compute, [model], window.counts, 'ldpc_train')

    last = {'loss': None, 'sigma_b_loss': None, 'acc': None}

    def drain(epoch, bcnt, say):
        """Read the window back (its one synchronisation) and start the next one."""
        read = window.read()
        if read is None:
            return
        got, (n, right) = read
        last.update(loss=sum(row[1] for row in got) / len(got), sigma_b_loss=sum(row[2] for row in got) / len(got),
                    acc=right / n if n else None)
        if say:
            print('epoch = {} bcnt = {} loss = {} acc = {} sigma_b_loss = {}'.format(epoch, bcnt, last['loss'], last['acc'],
                                                                                    last['sigma_b_loss']), flush=True)

    os.makedirs(out_dir, exist_ok=True)
    saved_to = None

    def save(epoch):
        nonlocal saved_to
        saved_to = checkpoint_path(out_dir, model_name, epoch, snr)
        torch.save(checkpoint_dict(model, opt, sched, epoch, gcnt, code), saved_to)

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
            full = window.push(keep['parts'])
            opt.step()
            gcnt += 1
            steps += 1
            if (log_every and gcnt % log_every == 0) or full:      # the script's `if gcnt % 10 == 0` (train_ldpc.py:242)
                drain(epoch, bcnt, bool(log_every))
        torch.cuda.synchronize(dev)
        seconds += time.perf_counter() - t0
        sched.step()
    drain(n_epochs - 1, steps_per_epoch - 1, False)      # the steps behind the last line: a last, shorter window
    if start_epoch < n_epochs:
        save(n_epochs)
    result = {'model_name': model_name, 'loss': last['loss'], 'sigma_b_loss': last['sigma_b_loss'], 'acc': last['acc'], 'losses': window.losses,
              'steps': steps, 'gcnt': gcnt, 'seconds': seconds, 'graphed': graphed is not None, 'checkpoint': saved_to}
    if test_set is not None:
        from .ldpc_eval import evaluate
        res = evaluate(model, test_set, dtype=dtype, code=code)
        result.update(ber=res['ber'], err_class=res['err_class'])
        print(res['ber'])
        print(torch.FloatTensor(res['err_class']))
    return result


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m fgnn_amd.ldpc_train',
                                 description="Train an LDPC decoder on batches drawn on the GPU (train_ldpc.py's training loop) and "
                                             "write the script's checkpoints.")
    ap.add_argument('--n_epochs', type=int, default=10)
    ap.add_argument('--batch_size', type=int, default=32)
    ap.add_argument('--snr', type=int, default=None, help='one SNR (dB) for every word; default: 0..4 dB per word')
    ap.add_argument('--aggregator', default='max')
    ap.add_argument('--model_path', default=None, help='resume from this checkpoint')
    ap.add_argument('--model_name', default='FactorNN')
    ap.add_argument('--steps_per_epoch', type=int, default=None, help='default: ceil(10000 / batch_size)')
    ap.add_argument('--dtype', choices=('bf16', 'f32'), default='bf16')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out_dir', default='.', help='where the checkpoints go')
    ap.add_argument('--save_every', type=int, default=SAVE_EVERY)
    ap.add_argument('--log_every', type=int, default=LOG_EVERY)
    ap.add_argument('--no-graph', dest='graph', action='store_false', help='eager steps, no hipGraph replay')
    ap.add_argument('--test_path', default=None, help='test set to evaluate on after the last epoch (ldpc_eval)')
    ap.add_argument('--code', default='builtin', help='builtin (96.3.963), the path of an alist file, or gallager:N,dv,dc,seed (dv = 3, dc = 6, N <= 96)')
    ap.add_argument('--json', action='store_true', help='print the result as one JSON line at the end')
    args = ap.parse_args(argv)
    from .ldpc_code import LdpcCode
    r = train(args.n_epochs, args.batch_size, args.snr, args.aggregator, trainloop.existing_or_none(args.model_path), args.model_name,
              args.steps_per_epoch, torch.bfloat16 if args.dtype == 'bf16' else torch.float32, args.seed, args.out_dir, args.save_every,
              args.log_every, args.graph, args.test_path, LR, 'cuda:0', LdpcCode.from_spec(args.code))
    if 'err_class' in r:                 # (an array: as lists for the JSON line; the last key either way)
        r['err_class'] = [[float(v) for v in row] for row in r['err_class']]
    trainloop.report(r, args.json)
    return 0


if __name__ == '__main__':
    sys.exit(main())
