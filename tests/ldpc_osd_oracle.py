"""numpy restatement of ordered-statistics reprocessing (csrc/ldpc_osd.hip, include/fgnn_hip_ldpc_osd.h), per word, integers throughout.

Per word (rel [N] f32 orders the positions and gives the hard decisions, metric [N] f32 scores the candidates; H in CSR form):

  q(v)     0 for a NaN, else uint32(min(|v|, 4096) * 256) in f32, truncated (at most 2^20)
  w = q(rel), h = rel < 0, wm = q(metric), hc = metric < 0 (a NaN gives 0 for all four); d = h ^ hc, sw = -wm where d else wm,
           C0 = sum wm d.  A candidate x costs sum wm (x ^ hc).
  viol given and 0: x = h, cost = C0, pattern = -1.
  order    the positions sorted by (w[n], n) ascending
  elimination   Gauss-Jordan over GF(2) of [H | s], s = H h, the columns in that order: a column is a pivot exactly when a row not yet
           used has a one in it (here: the lowest such row becomes the pivot row; the result does not depend on the choice) and is
           then cleared from every other row.  piv_i, s'_i, a_i(c) as in the header; f_j: the non-pivot columns in order.
  candidates    index 0 flips piv_i where s'_i; index 1 + j (j < L = min(span, N - rank), order >= 1) flips f_j and piv_i where
           s'_i ^ a_i(f_j); the pairs j < k in lexicographic order from 1 + L (order 2) flip f_j, f_k and piv_i where
           s'_i ^ a_i(f_j) ^ a_i(f_k).  Cost = C0 + sum sw over the flipped positions.
  result   the smallest (cost, index): x = h ^ flips, cost, pattern = index.

``eliminate`` does the part that does not depend on (order, span) once per word; ``candidates`` scores.  Pair costs are formed as
P_j + Q_k - 2 (U^T diag(psw) A)_jk with u = s' ^ a, which is sum psw (u_j ^ a_k) in exact int64 arithmetic.  Every returned x is
checked here: H x = 0 and cost = sum wm (x ^ hc)."""
import numpy as np


def quantise(v):
    v = np.asarray(v, np.float32)
    nan = np.isnan(v)
    a = np.minimum(np.abs(np.where(nan, np.float32(0), v)), np.float32(4096.0)) * np.float32(256.0)
    return np.where(nan, 0, a.astype(np.uint32)).astype(np.int64)


def dense(row_ptr, row_var, N):
    """H [M, N] uint8 from its CSR tables."""
    M = len(row_ptr) - 1
    H = np.zeros((M, N), np.uint8)
    for m in range(M):
        H[m, np.asarray(row_var[row_ptr[m]:row_ptr[m + 1]], np.int64)] ^= 1
    return H


def eliminate(rel, metric, H):
    """One word's state after the elimination (a dict): h, hc, wm, sw, C0, order, piv, free, A [rank, N] uint8, s [rank]."""
    rel = np.asarray(rel, np.float32)
    metric = rel if metric is None else np.asarray(metric, np.float32)
    M, N = H.shape
    with np.errstate(invalid='ignore'):
        h, hc = (rel < 0).astype(np.uint8), (metric < 0).astype(np.uint8)
    w, wm = quantise(rel), quantise(metric)
    d = h ^ hc
    sw = np.where(d == 1, -wm, wm)
    C0 = int((wm * d).sum())
    order = np.lexsort((np.arange(N), w))
    W = (N + 1 + 63) // 64
    aug = np.concatenate([H, (H.astype(np.int64) @ h.astype(np.int64) % 2).astype(np.uint8)[:, None]], 1)
    rows = np.packbits(np.pad(aug, ((0, 0), (0, 64 * W - (N + 1)))), axis=1, bitorder='little').view(np.uint64)      # [M, W]
    used = np.zeros(M, bool)
    piv, prow, free = [], [], []
    for c in order:
        c = int(c)
        bit = (rows[:, c >> 6] >> np.uint64(c & 63)) & np.uint64(1) != 0
        el = np.nonzero(bit & ~used)[0]
        if el.size == 0:
            free.append(c)
            continue
        p = int(el[0])
        bit[p] = False
        rows[bit] ^= rows[p]
        used[p] = True
        piv.append(c)
        prow.append(p)
    full = np.unpackbits(rows.view(np.uint8), axis=1, bitorder='little')[:, :N + 1]
    assert not full[~used].any()                                         # unused rows end all-zero, syndrome included
    A = full[np.asarray(prow, np.int64)] if prow else np.zeros((0, N + 1), np.uint8)
    return {'h': h, 'hc': hc, 'wm': wm, 'sw': sw, 'C0': C0, 'order': order, 'piv': np.asarray(piv, np.int64),
            'free': np.asarray(free, np.int64), 'A': A[:, :N], 's': A[:, N].astype(np.int64), 'H': H}


def candidates(st, order, span):
    """(x [N] uint8, cost, pattern) of one reprocessed word."""
    assert order in (0, 1, 2) and span >= 1
    piv, free, s, sw, C0 = st['piv'], st['free'], st['s'], st['sw'], st['C0']
    L = min(int(span), len(free))
    psw = sw[piv]
    costs = [np.array([C0 + int((s * psw).sum())], np.int64)]
    Af = st['A'][:, free[:L]].astype(np.int64)                            # [rank, L]
    U = s[:, None] ^ Af
    if order >= 1:
        costs.append(C0 + sw[free[:L]] + (U * psw[:, None]).sum(0))
    if order == 2 and L >= 2:
        P = sw[free[:L]] + (U * psw[:, None]).sum(0)
        Q = sw[free[:L]] + (Af * psw[:, None]).sum(0)
        pair = C0 + P[:, None] + Q[None, :] - 2 * ((U * psw[:, None]).T @ Af)
        j, k = np.triu_indices(L, 1)                                      # row-major: lexicographic
        costs.append(pair[j, k])
    costs = np.concatenate(costs)
    idx = int(np.argmin(costs))                                           # the first smallest
    flips = np.zeros(len(sw), np.uint8)
    col = s.copy()
    if 1 <= idx <= L:
        cols = [idx - 1]
    elif idx > L:
        cols = [int(j[idx - 1 - L]), int(k[idx - 1 - L])]
    else:
        cols = []
    for t in cols:
        flips[free[t]] ^= 1
        col = col ^ Af[:, t]
    flips[piv[col == 1]] = 1
    x = st['h'] ^ flips
    cost = int(costs[idx])
    assert not (st['H'].astype(np.int64) @ x.astype(np.int64) % 2).any()
    assert cost == int((st['wm'] * (x ^ st['hc'])).sum())
    return x, cost, idx


def states(rel, metric, H, viol=None):
    """``eliminate`` per word of a batch (None for a pass-through word): compute once, share among (order, span)."""
    rel = np.asarray(rel, np.float32)
    return [None if viol is not None and viol[b] == 0 else eliminate(rel[b], None if metric is None else metric[b], H)
            for b in range(rel.shape[0])]


def reprocess(rel, metric, viol, H, order, span, sts=None):
    """The batch: rel [B, N], metric [B, N] or None, viol [B] or None.  Returns (x [B, N] uint8, cost [B] int32, pattern [B] int32)."""
    rel = np.asarray(rel, np.float32)
    B, N = rel.shape
    sts = states(rel, metric, H, viol) if sts is None else sts
    x, cost, pattern = np.zeros((B, N), np.uint8), np.zeros(B, np.int32), np.zeros(B, np.int32)
    for b in range(B):
        if viol is not None and viol[b] == 0:
            m = rel[b] if metric is None else np.asarray(metric[b], np.float32)
            with np.errstate(invalid='ignore'):
                h, hc = (rel[b] < 0).astype(np.uint8), (m < 0).astype(np.uint8)
            x[b], cost[b], pattern[b] = h, int((quantise(m) * (h ^ hc)).sum()), -1
        else:
            x[b], cost[b], pattern[b] = candidates(sts[b], order, span)
    return x, cost, pattern


def bp_osd(llr, tabs, layers, H, order, span, algorithm='min-sum', max_iter=20, **kw):
    """The composition ``ldpc_decoders.Decoder.run`` runs: ``ldpc_llr_oracle.decode``, then reprocessing of its posteriors against the
    channel LLRs, the words it finished passed through.  Returns (x, cost, pattern, the decoder's result)."""
    import ldpc_llr_oracle as LO
    r = LO.decode(llr, tabs, layers, algorithm, max_iter, **kw)
    return reprocess(r['post'], llr, r['viol'], H, order, span) + (r,)
