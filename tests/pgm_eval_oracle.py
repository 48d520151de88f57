"""numpy restatement of csrc/pgm_eval.hip (scores of decisions on the synthetic-PGM chain models) and of the arithmetic of the
reference's synthetic test loops (train_syn_hop_factor.py:349-409 and its two siblings), plus those loops' statements run literally
on torch CPU tensors, to hold the restatement to.

Arrays carry a leading batch axis: logits [B, 2, N] (class axis 1, the model's [B, 2, N, 1] without its last axis), assignments
[B, N], labels [B, N], unary [B, N, 2], pair [B, N-1, 4] (row-major [x_i][x_{i+1}]), caps [B, N-h+1]."""
import statistics

import numpy as np
import torch


def decisions(logits):
    """torch.argmax over the class axis of [B, 2, N] f32 logits: the first maximum, NaN above every number."""
    v0, v1 = logits[:, 0].astype(np.float32), logits[:, 1].astype(np.float32)
    return ((v1 > v0) | (np.isnan(v1) & ~np.isnan(v0))).astype(np.int64)


def score(dec, label, unary, pair, caps, h, logits=True):
    """(correct [B] int, feasible [B] bool, objective [B] f64, nll [B] f64 or None) as the kernel forms them: x = the argmax of
    the logits or (assignment != 0); correct where x == label (logits) / assignment == label; the objective summed in f64 in the
    MAP recursion's order u_0, then (acc + pair_{t-1}) + u_t; nll = sum_i logsumexp(v0, v1) - v_label in f64."""
    label = np.asarray(label, np.int64)
    B, N = label.shape
    if logits:
        dec = np.asarray(dec, np.float32)
        x = decisions(dec)
        correct = (x == label).sum(1)
    else:
        a = np.asarray(dec, np.int64)
        x = (a != 0).astype(np.int64)
        correct = (a == label).sum(1)
    unary = np.asarray(unary, np.float32).astype(np.float64)
    pair = np.asarray(pair, np.float32).astype(np.float64)
    caps = np.asarray(caps, np.int64)
    rows = np.arange(B)
    obj = unary[rows, 0, x[:, 0]]
    for t in range(1, N):
        obj = (obj + pair[rows, t - 1, 2 * x[:, t - 1] + x[:, t]]) + unary[rows, t, x[:, t]]
    cs = np.concatenate([np.zeros((B, 1), np.int64), np.cumsum(x, 1)], 1)
    win = cs[:, h:] - cs[:, :N - h + 1]
    feasible = (win <= caps).all(1)
    nll = None
    if logits:
        a, c = dec[:, 0].astype(np.float64), dec[:, 1].astype(np.float64)
        with np.errstate(invalid='ignore', over='ignore'):
            lse = np.where(a > c, a, c) + np.log1p(np.exp(-np.abs(a - c)))
            nll = (lse - np.where(label != 0, c, a)).sum(1)
    return correct, feasible, obj, nll


def loop_figures(correct, lp_correct, nll, N, batch_size):
    """The figures of the reference's test loop from per-sample counts in file order, batches of batch_size (the last may be
    short): (acc, acc_lp, stddev, stddev_lp, mean loss) with acc = the running sum of per-batch accuracies / number of batches."""
    n = len(correct)
    acc, acc_lp, loss = [], [], []
    for s in range(0, n, batch_size):
        e = min(n, s + batch_size)
        acc.append(int(np.sum(correct[s:e])) / ((e - s) * N))
        acc_lp.append(int(np.sum(lp_correct[s:e])) / ((e - s) * N))
        if nll is not None:
            loss.append(float(np.sum(nll[s:e])) / ((e - s) * N))
    sa = sl = 0
    for a, b in zip(acc, acc_lp):
        sa += a
        sl += b
    return sa / len(acc), sl / len(acc), statistics.stdev(acc), statistics.stdev(acc_lp), (np.mean(loss) if loss else None)


def reference_loop(batches):
    """train_syn_hop_factor.py:349-409's statements, literally, over (pred [b, 2, N, 1] model output, nlabel [b, N], lp_label
    [b, N]) torch CPU batches: returns (accum_acc / gcnt, accum_acc_lp / gcnt, stdev(acc_global), stdev(acc_lp_global), the mean
    of every batch's loss.item())."""
    loss_seq, acc_global, acc_lp_global = [], [], []
    gcnt = 0
    accum_acc = 0
    accum_acc_lp = 0
    for pred, nlabel, lp_label in batches:
        pred = pred.squeeze(-1).permute(0, 2, 1).contiguous()
        loss = torch.nn.functional.cross_entropy(pred.view(-1, 2), nlabel.view(-1))
        loss_seq.append(loss.item())
        gcnt += 1
        pred_int = pred.argmax(dim=-1)
        all_correct = torch.sum(pred_int == nlabel)
        lp_correct = torch.sum(lp_label == nlabel)
        acc = all_correct.item() / np.prod(nlabel.shape)
        lp_acc = lp_correct.item() / np.prod(nlabel.shape)
        acc_global.append(acc)
        acc_lp_global.append(lp_acc)
        accum_acc += acc
        accum_acc_lp += lp_acc
    return (accum_acc / gcnt, accum_acc_lp / gcnt, statistics.stdev(acc_global), statistics.stdev(acc_lp_global),
            float(np.mean(loss_seq)))
