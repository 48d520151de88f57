"""A numpy restatement of the reference's LDPC test accounting (/root/reference/train_ldpc.py:289-327), the checker of
csrc/ldpc_eval.hip (fgnn_ldpc_error_counts).

Per batch the reference takes pred_int = (pred >= 0), classifies each word by the SNR of its bit 0 (|snr - csnr| < 1e-3 in f32) and
by sigma_b.long() (truncation), and adds, per class, the message bits right (acc_cnt) and compared (acc_tot = words x 48); overall it
adds the bits right (acc_seq) and compared (tot).  Here the same as integer counts: rows SNR-major, the last row over every word;
columns {bits compared, bit errors, words, word errors} (word errors: no reference counterpart)."""
import numpy as np


def decisions(v, kind):
    """Hard bits of the decisions: logits (f32, or bf16 given as their f32 values): v >= 0 (-0 counts as 1); bytes: v != 0."""
    v = np.asarray(v)
    return (v >= 0).astype(np.int64) if kind == 'logits' else (v != 0).astype(np.int64)


def classes(snr_first, sigma_b, snr_grid, sigma_grid):
    """Class row per word (-1: none): the first SNR grid value within 1e-3 (f32 arithmetic) and the sigma grid value equal to the
    truncated sigma_b."""
    snr = np.asarray(snr_first, np.float32)
    sb = np.trunc(np.asarray(sigma_b, np.float64))
    si = np.full(snr.shape, -1, np.int64)
    for k in range(len(snr_grid) - 1, -1, -1):                 # the first match wins
        si[np.abs(snr - np.float32(snr_grid[k])) < np.float32(1e-3)] = k
    bi = np.full(snr.shape, -1, np.int64)
    for k in range(len(sigma_grid) - 1, -1, -1):
        bi[sb == sigma_grid[k]] = k
    return np.where((si >= 0) & (bi >= 0), si * len(sigma_grid) + bi, -1)


def error_counts(dec, kind, label, snr_first, sigma_b, snr_grid=(0, 1, 2, 3, 4), sigma_grid=(0, 1, 2, 3, 4, 5), nbits=48):
    """counts [n_snr * n_sigma + 1, 4] int64 of one batch."""
    bits = decisions(np.asarray(dec)[:, :nbits], kind)
    lab = np.asarray(label)[:, :nbits].astype(np.int64)
    wrong = bits != lab
    errs = wrong.sum(1)
    cls = classes(snr_first, sigma_b, snr_grid, sigma_grid)
    out = np.zeros((len(snr_grid) * len(sigma_grid) + 1, 4), np.int64)
    for r in range(out.shape[0] - 1):
        m = cls == r
        out[r] = (m.sum() * nbits, errs[m].sum(), m.sum(), (errs[m] > 0).sum())
    out[-1] = (len(errs) * nbits, errs.sum(), len(errs), (errs > 0).sum())
    return out


def reference_loop(pred, label, cur_snr, sigma_b, snr_grid=(0, 1, 2, 3, 4), n_sigma=6):
    """The reference's own loop body (train_ldpc.py:302-323) on torch CPU tensors, literally: (acc_cnt, acc_tot, all_correct, tot)."""
    import torch
    acc_cnt = np.zeros((len(snr_grid), n_sigma))
    acc_tot = np.zeros((len(snr_grid), n_sigma))
    pred_int = (pred >= 0).long().squeeze()
    label = label.squeeze()
    for i, csnr in enumerate(snr_grid):
        for b in range(n_sigma):
            indice = (sigma_b.long() == b) & (abs(cur_snr - csnr) < 1e-3)
            acc_cnt[i][b] += torch.sum(pred_int[indice, :48] == label[indice, :48]).item()
            acc_tot[i][b] += torch.sum(indice) * 48
    all_correct = torch.sum(pred_int[:, :48] == label[:, :48]).item()
    return acc_cnt, acc_tot, all_correct, np.prod(label.shape) // 2
