"""Training synthetic-PGM MAP models on the GPU: the loop of the reference's synthetic scripts, from sampling to the checkpoint.

The reference's training loop (/root/reference/train_syn_hop_factor.py:250-330, train_syn_pw_factor.py:250-330,
train_syn_fixed_pw_hop.py:236-312) reads an AD3-labelled pickle, runs the model, takes the cross entropy against the MAP label,
clips the gradient norm to 1, steps Adam at 3e-3 under ``LambdaLR(max(0.98**epoch, 1e-6))`` and saves a checkpoint every epoch.
Here every batch is drawn and labelled on the device (``PgmDataPath.sample(batch_size, family, seed, step=gcnt)``), the loss and the
per-step accuracy counts are one kernel (``labelling_loss``, csrc/pgm_loss.hip), the clip rides inside the one-kernel Adam
(``FastAdam(max_grad_norm=1.0)``, csrc/flat_adam.hip), the forward / loss / backward are replayed as one hipGraph, and the host
reads nothing back between log lines.  The checkpoints are the scripts' dicts: ``pgm_eval.load_checkpoint`` reads them and an
unchanged ``train_syn_*.py --model_path`` resumes from them.

``python -m fgnn_amd.pgm_train --family hops --train_epoches 20`` is the command line.
"""
import argparse
import os
import sys
import time
import warnings

import torch

from . import _hip, trainloop
from .pgm_datapath import FAMILIES
from .pgm_eval import CAP, EDGE_KEYS, HOP_ORDER, MODEL_NAMES, TRANSITION, _check_family, build_model, run_batch

LR = 3e-3                            # every script's Adam
MAX_GRAD_NORM = 1.0                  # ... and its clip_grad_norm(parameters, 1.0)
TRAIN_SIZE = 90000                   # ... and its --train_size: an epoch is ceil(TRAIN_SIZE / batch_size) steps
CHAIN_LENGTH = 30                    # --chain_length
MAXN = 1024                          # csrc/pgm_loss.hip: PL_MAXN


def lr_lambda(x):
    """The scripts' ``LambdaLR`` factor."""
    return max(0.98 ** x, 1e-6)


def default_steps_per_epoch(batch_size):
    """Batches of a DataLoader over the scripts' 90000 training items (the last one may be short there; here every batch is full)."""
    batch_size = int(batch_size)
    if batch_size < 1:
        raise ValueError('batch_size must be >= 1')
    return -(-TRAIN_SIZE // batch_size)


def epoch_lr(epoch):
    """The rate 0-based epoch ``epoch`` trains at: the scripts step the scheduler at the top of every epoch, before its first batch."""
    return LR * lr_lambda(epoch + 1)


class _LabellingLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, label, lp_label, counts):
        B, _, N = pred.shape
        L = _hip.lib()
        loss = torch.empty((), device=pred.device, dtype=torch.float32)
        ws = torch.empty(int(L.fgnn_pgm_loss_workspace_bytes()) // 8, device=pred.device, dtype=torch.float64)
        kind = _hip.PGM_DEC_F32 if pred.dtype == torch.float32 else _hip.PGM_DEC_BF16
        sb, cs, vs = pred.stride()
        _hip.call('fgnn_pgm_loss_forward', pred, kind, sb, cs, vs, label, label.stride(0), lp_label,
                  0 if lp_label is None else lp_label.stride(0), B, N, loss, counts, ws, ws.numel() * 8)
        ctx.save_for_backward(pred, label)
        ctx.kind = kind
        return loss

    @staticmethod
    def backward(ctx, gloss):
        pred, label = ctx.saved_tensors
        B, _, N = pred.shape
        g = torch.empty((B, 2, N), device=pred.device, dtype=pred.dtype)
        gloss = gloss.reshape(1).float().contiguous()
        sb, cs, vs = pred.stride()
        _hip.call('fgnn_pgm_loss_backward', pred, ctx.kind, sb, cs, vs, label, label.stride(0), gloss, B, N, g, *g.stride())
        return g, None, None, None


def labelling_loss(pred, label, lp_label=None, counts=None):
    """``F.cross_entropy(pred.squeeze(-1).permute(0, 2, 1).reshape(-1, 2), label.view(-1))`` — the scripts' loss — as a 0-dim f32
    tensor with a backward, from the model's output as it is (csrc/pgm_loss.hip: two short launches forward, one backward).

    pred: logits [B, 2, N, 1] or [B, 2, N], f32 or bf16, any strides.  label [B, N] int64, the exact MAP.  ``counts`` [3] int64 on
    pred's device, if given, is ADDED to: variables, variables where ``argmax(pred)`` equals the label, variables where ``lp_label``
    ([B, N] int64, optional) equals it — the scripts' per-step ``acc`` / ``lp_acc`` without a host read.  Bad shapes or dtypes raise
    ValueError before anything reaches the device; anything but a ROCm device raises RuntimeError (no CPU fallback)."""
    if label.dim() != 2 or label.dtype != torch.int64:
        raise ValueError('label must be [B, N] int64, got %s %s' % (tuple(label.shape), label.dtype))
    B, N = label.shape
    if pred.dtype not in (torch.float32, torch.bfloat16):
        raise ValueError('logits must be f32 or bf16, got %s' % pred.dtype)
    if pred.dim() == 4 and pred.shape[3] == 1:
        pred = pred[..., 0]
    if pred.dim() != 3 or tuple(pred.shape) != (B, 2, N):
        raise ValueError('logits must be [%d, 2, %d, 1] or [%d, 2, %d], got %s' % (B, N, B, N, tuple(pred.shape)))
    if not 1 <= N <= MAXN:
        raise ValueError('chain length N = %d outside 1..%d' % (N, MAXN))
    if lp_label is not None and (lp_label.dtype != torch.int64 or tuple(lp_label.shape) != (B, N)):
        raise ValueError('lp_label must be [%d, %d] int64, got %s %s' % (B, N, tuple(lp_label.shape), lp_label.dtype))
    if counts is not None and (counts.dtype != torch.int64 or tuple(counts.shape) != (3,) or counts.device != pred.device
                               or not counts.is_contiguous()):
        raise ValueError('counts must be a contiguous [3] int64 tensor on %s' % pred.device)
    if not pred.is_cuda:
        raise RuntimeError('labelling_loss runs on a ROCm device (no CPU fallback)')
    dense = lambda t: t if t is None or (t.device == pred.device and (t.stride(1) == 1 or N == 1)) else t.to(pred.device).contiguous()
    return _LabellingLoss.apply(pred, dense(label), dense(lp_label), counts)


def checkpoint_dict(family, model, edge_models, optimizer, scheduler, epoch, gcnt):
    """The dict the family's script saves (``get_model_dict``, train_syn_hop_factor.py:249-258): the model's and the edge models'
    state dicts under the family's keys, the optimizer's (stock Adam's layout) and the scheduler's, the epoch and the step count."""
    _check_family(family)
    d = {'model_state_dict': model.state_dict()}
    for m, k in zip(edge_models, EDGE_KEYS[family]):
        d[k] = m.state_dict()
    d.update(optimizer_state_dict=optimizer.state_dict(), lr_sche=scheduler.state_dict(), epoch=int(epoch), gcnt=int(gcnt))
    return d


def checkpoint_path(out_dir, family, model_name, epoch):
    return os.path.join(out_dir, '%s_%s_epoches_%d.pt' % (model_name, family, epoch))


def _scheduler(opt):
    return torch.optim.lr_scheduler.LambdaLR(opt, lr_lambda=lr_lambda)


def train(family, epochs, batch_size=32, steps_per_epoch=None, seed=0, model_name=None, model_path=None, out_dir='.',
          lp_label=False, graph=True, log_every=10, device='cuda'):
    """Train the family's model (``pgm_eval.build_model``) for ``epochs`` epochs of ``steps_per_epoch`` batches (default: the
    scripts' ceil(90000 / batch_size)); batch number ``gcnt`` (counted from 0 over the whole run, resumes included) is
    ``PgmDataPath.sample(batch_size, family, seed, step=gcnt)`` with ``pgm_eval``'s CAP / TRANSITION / HOP_ORDER, so no batch is shared
    with a ``make_test_set`` test set.  Loss ``labelling_loss``, optimizer ``FastAdam(lr=3e-3, max_grad_norm=1.0)`` over the model's
    and the edge models' parameters, ``LambdaLR(max(0.98**x, 1e-6))`` stepped at the top of every epoch (epoch e trains at
    ``epoch_lr(e)``).  ``seed`` also seeds the parameter initialisation.

    As the scripts do, a checkpoint (``checkpoint_dict``) is written at the top of every epoch and after the last one, to
    ``checkpoint_path(out_dir, family, model_name, epoch)``; ``model_path`` resumes from one: parameters, Adam state, scheduler,
    epoch and ``gcnt`` (the Philox steps continue where they stopped).

    ``graph``: the forward, loss and backward are captured once (``graph.StepGraph``) and replayed, every batch copied into the
    captured input buffers; the norm launches and the clipped Adam follow eagerly.  A capture failure falls back to eager steps with
    one line on stderr.  Nothing is read back per step: the losses go into a device ring and the accuracy counts accumulate on the
    device; both are read every ``log_every`` steps for the log line ``epoch bcnt loss acc [lp_acc]`` (``lp_label``: draw the
    LP-relaxation label too and report its accuracy, as the scripts do; 0 / None: no log lines).

    Returns a dict: loss and acc (lp_acc) of the last log window, losses (every step's, f32 values), steps, gcnt, seconds (the step
    loops, without the checkpoint writes), graphed, checkpoint (the last one's path)."""
    _check_family(family)
    epochs, batch_size, seed = int(epochs), int(batch_size), int(seed)
    steps_per_epoch = default_steps_per_epoch(batch_size) if steps_per_epoch is None else int(steps_per_epoch)
    if epochs < 0 or batch_size < 1 or steps_per_epoch < 1:
        raise ValueError('epochs >= 0, batch_size >= 1 and steps_per_epoch >= 1 needed')
    model_name = model_name or MODEL_NAMES[family][0]
    dev = trainloop.cuda_device(device)
    from .fastpath import FastAdam
    from .pgm_datapath import PgmDataPath

    torch.manual_seed(seed)
    model, edge = build_model(family, model_name)
    ckpt = None
    if model_path:
        ckpt = torch.load(model_path, map_location='cpu', weights_only=True)
        model.load_state_dict(ckpt['model_state_dict'], strict=True)
        for m, k in zip(edge, EDGE_KEYS[family]):
            m.load_state_dict(ckpt[k], strict=True)
    mods = [model] + list(edge)
    for m in mods:
        m.to(dev).train()
    params = [p for m in mods for p in m.parameters()]
    opt = FastAdam(params, lr=LR, max_grad_norm=MAX_GRAD_NORM)
    sched = _scheduler(opt)
    start_epoch, gcnt = (0, 0) if ckpt is None else trainloop.resume(ckpt, opt, sched)
    path = PgmDataPath(dev, CHAIN_LENGTH, HOP_ORDER)
    nfeat = {'raw': 1, 'pws': 2, 'hops': 3}[family]
    draw = lambda step: path.sample(batch_size, family, seed, step=step, cap=CAP, transition=TRANSITION, lp_label=lp_label)

    window = trainloop.LogWindow(dev, 1, 3, log_every)       # rows {loss}; counts {variables, argmax == label, LP label == label}
    keep = {}

    def compute(batch):
        feats, label, lp = batch[:nfeat], batch[nfeat], batch[nfeat + 1] if lp_label else None
        opt.zero_grad()
        pred = run_batch(model, edge, family, feats, HOP_ORDER)
        loss = labelling_loss(pred, label, lp, window.counts)
        loss.backward()
        keep['loss'] = loss.detach()

    graphed, static = None, None
    if graph and start_epoch < epochs:
        static = [t.clone() for t in draw(gcnt)]
        graphed = trainloop.capture_step(lambda: compute(static), mods, window.counts, 'pgm_train')

    last = {'loss': None, 'acc': None, 'lp_acc': None}

    def drain(epoch, bcnt, say):
        """Read the window back (its one synchronisation) and start the next one."""
        read = window.read()
        if read is None:
            return
        rows, (n, right, lp_right) = read
        got = [row[0] for row in rows]
        last.update(loss=sum(got) / len(got), acc=right / n if n else None, lp_acc=lp_right / n if n and lp_label else None)
        if say:
            line = 'epoch = {} bcnt = {} loss = {} acc = {}'.format(epoch, bcnt, last['loss'], last['acc'])
            print(line + (' lp_acc = {}'.format(last['lp_acc']) if lp_label else ''), flush=True)

    os.makedirs(out_dir, exist_ok=True)
    saved_to = None

    def save(epoch):
        nonlocal saved_to
        saved_to = checkpoint_path(out_dir, family, model_name, epoch)
        torch.save(checkpoint_dict(family, model, edge, opt, sched, epoch, gcnt), saved_to)

    seconds, steps = 0.0, 0
    for epoch in range(start_epoch, epochs):
        save(epoch)
        with warnings.catch_warnings():      # (the scripts step the scheduler before the epoch's first optimizer step, on purpose)
            warnings.filterwarnings('ignore', message='Detected call of `lr_scheduler.step\\(\\)` before')
            sched.step()
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        for bcnt in range(steps_per_epoch):
            batch = draw(gcnt)
            if graphed is not None:
                for st, t in zip(static, batch):
                    st.copy_(t)
                graphed.replay()
            else:
                compute(batch)
            full = window.push(keep['loss'])
            opt.step()
            gcnt += 1
            steps += 1
            if full:
                drain(epoch, bcnt, bool(log_every))
        drain(epoch, steps_per_epoch - 1, False)
        torch.cuda.synchronize(dev)
        seconds += time.perf_counter() - t0
    if start_epoch < epochs:
        save(epochs)
    return {'family': family, 'model_name': model_name, 'loss': last['loss'], 'acc': last['acc'], 'lp_acc': last['lp_acc'],
            'losses': window.losses, 'steps': steps, 'gcnt': gcnt, 'seconds': seconds, 'graphed': graphed is not None,
            'checkpoint': saved_to}


def main(argv=None):
    ap = argparse.ArgumentParser(prog='python -m fgnn_amd.pgm_train',
                                 description="Train a synthetic-PGM model on batches drawn on the GPU (train_syn_*.py's training "
                                             "loop) and write the scripts' checkpoints.")
    ap.add_argument('--family', choices=sorted(FAMILIES), default='hops')
    ap.add_argument('--train_epoches', type=int, default=20)
    ap.add_argument('--batch_size', type=int, default=32)
    ap.add_argument('--steps_per_epoch', type=int, default=None, help='default: ceil(90000 / batch_size)')
    ap.add_argument('--model_path', default=None, help='resume from this checkpoint')
    ap.add_argument('--model_name', default=None, help='raw: mp_nn (default), mp_nn_comp, simple_gnn, iid; pws / hops: mp_nn_factor')
    ap.add_argument('--seed', type=int, default=0)
    ap.add_argument('--out_dir', default='.', help='where the checkpoints go')
    ap.add_argument('--lp_label', action='store_true', help='draw the LP-relaxation label too and log lp_acc')
    ap.add_argument('--no-graph', dest='graph', action='store_false', help='eager steps, no hipGraph replay')
    ap.add_argument('--log_every', type=int, default=10)
    ap.add_argument('--json', action='store_true', help='print the result as one JSON line at the end')
    args = ap.parse_args(argv)
    r = train(args.family, args.train_epoches, args.batch_size, args.steps_per_epoch, args.seed, args.model_name,
              trainloop.existing_or_none(args.model_path), args.out_dir, args.lp_label, args.graph, args.log_every, 'cuda:0')
    trainloop.report(r, args.json)
    return 0


if __name__ == '__main__':
    sys.exit(main())
