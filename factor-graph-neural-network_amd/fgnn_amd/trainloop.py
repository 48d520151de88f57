"""What the training loops share (``ldpc_train.train``, ``pgm_train.train``): the device they run on, the resume, the capture
with its eager fallback, the device-side log window and the ends of the command lines.  The epoch loops stay in the trainers:
when the scheduler steps, when a checkpoint is written, when a window ends and how a batch reaches the captured buffers differ.
"""
import json
import os
import sys

import torch

from . import graph


def cuda_device(device):
    """``device`` as a ``torch.device`` with an index; anything but a ROCm device raises RuntimeError."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise RuntimeError('train runs on a ROCm device (no CPU fallback)')
    if dev.index is None:
        dev = torch.device('cuda', torch.cuda.current_device())
    return dev


def resume(ckpt, opt, sched):
    """Adam's state and the scheduler's from a checkpoint dict (the model's state dicts are the caller's: their keys differ);
    returns the checkpoint's (epoch, gcnt)."""
    opt.load_state_dict(ckpt['optimizer_state_dict'])
    sched.load_state_dict(ckpt['lr_sche'])
    graph.state_moved()
    return int(ckpt['epoch']), int(ckpt['gcnt'])


def capture_step(compute, modules, counts, who):
    """``graph.StepGraph(compute, modules=modules)``, or None after one line on stderr, with ``who`` as its prefix, when the
    capture raises.  ``counts``: the tensor the step's loss kernel adds to; the warm-up runs were real steps."""
    graphed = None
    try:
        graphed = graph.StepGraph(compute, modules=modules)
    except Exception as e:               # noqa: BLE001 — report and fall back to eager launches
        print('%s: hipGraph capture failed (%s: %s); running eagerly' % (who, type(e).__name__, e), file=sys.stderr)
    finally:                             # replays and eager steps alike start from the counts (and buffers) of graph=False
        counts.zero_()
        graph.state_moved()
    return graphed


class LogWindow:
    """The steps since the last read, kept on the device: a ring with one row of ``columns`` f32 values per step (column 0: the
    step's loss) and ``counters`` int64 ``counts`` that the loss kernel adds to.  ``counts`` is allocated once and only ever
    zeroed in place: a captured step holds its address.  The ring has ``log_every`` rows (0 / None: 256)."""

    def __init__(self, device, columns, counters, log_every):
        self.counts = torch.zeros(counters, dtype=torch.int64, device=device)
        self.ring = torch.zeros((int(log_every) if log_every else 256, columns), dtype=torch.float32, device=device)
        self.pending, self.losses = 0, []

    def push(self, row):
        """Copy a step's row in (no host read); True when the ring is full, and has to be read before the next push."""
        self.ring[self.pending].copy_(row)
        self.pending += 1
        return self.pending == len(self.ring)

    def read(self):
        """(rows, counts) as Python lists — the one synchronisation of a window — and a new window: ``counts`` zeroed, column 0
        of the rows appended to ``losses``.  None when no step is pending."""
        if not self.pending:
            return None
        rows, counts = self.ring[:self.pending].tolist(), self.counts.tolist()
        self.counts.zero_()
        self.pending = 0
        self.losses.extend(row[0] for row in rows)
        return rows, counts


def existing_or_none(model_path):
    """A command line's ``--model_path``: the reference scripts' default is a path that need not exist."""
    return model_path if model_path and os.path.exists(model_path) else None


def report(result, as_json):
    """The last line of a command line: ``train``'s result without its per-step ``losses`` as one JSON line, or a sentence."""
    if as_json:
        print(json.dumps({k: v for k, v in result.items() if k != 'losses'}))
    else:
        print('training done: {} steps in {:.2f} s, loss = {}, acc = {}, checkpoint {}'.format(
            result['steps'], result['seconds'], result['loss'], result['acc'], result['checkpoint']))
