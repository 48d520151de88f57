"""numpy restatement of the LLR-domain LDPC decoders (csrc/ldpc_llr.hip, include/fgnn_hip_ldpc_llr.h), vectorised over the batch.

The steps, in the order of their operations (``dtype`` float32 restates the kernel's arithmetic; float64 is the yardstick of the
sum-product comparison):

  load     prior[n] = llr[n] (read as f32); NaN -> 0; clamped to +-4096.  T[n] = prior[n], R[e] = 0.
  check m  over its edges l = 0 .. L-1 in row order:  q_l = T[row_var] - R[row_edge]; negative exactly when q_l < 0.
           0  R'_l = s_l (alpha min_{k != l} |q_k|), s_l the product of the other signs
           1  R'_l = s_l max(min_{k != l} |q_k| - beta, 0)
           2  t_l = tanh(0.5 q_l); F_0 = 1, F_{l+1} = F_l t_l; S_L = 1, S_l = S_{l+1} t_l; p_l = F_l S_{l+1} clamped to
              +-(1 - 2^-24); R'_l = 2 atanh(p_l)
           a check of degree 1 sends 0.
  flooding every check from the old T, R <- R'; then T[n] = prior[n] + R[col_ptr[n]] + R[col_ptr[n] + 1] + ... in that order.
  layered  the layers in order; a check stores R[e] = R'_l and T[var] = q_l + R'_l.
  after an iteration  x[n] = T[n] < 0, viol = checks of odd parity; a word stops at viol = 0 or at max_iter.

Overflow (min-sum on a code whose messages feed back, such as a 16 x 16 Gallager code under the layered schedule, can double T per
layer until it passes the f32 range): infinities follow IEEE; a NaN q (inf - inf) is skipped by the minimum, counts as non-negative
and makes the totals it enters NaN, whose hard decision is 0.

The checks of one pass (all of them, or one layer's) do not read what another of them writes, so they are updated together, grouped
by degree.  ``margin`` [B]: the smallest |T| over all variables and all iterations a word ran.
"""
import numpy as np

ALGORITHMS = {'min-sum': 0, 'offset-min-sum': 1, 'sum-product': 2}
CLAMP = 4096.0
PMAX = 1.0 - 2.0 ** -24


def tables(nlist, nchk):
    """alist column lists (each variable's checks in file order, -1 = padding) -> (col_ptr, row_ptr, row_edge, row_var), as
    ``LdpcCode.incidence_tables`` builds them (restated here on purpose)."""
    cols = [[int(m) for m in row if m >= 0] for row in nlist]
    col_ptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])]).astype(np.int64)
    rows = [[] for _ in range(nchk)]
    for n, c in enumerate(cols):
        for u, m in enumerate(c):
            rows[m].append((int(col_ptr[n]) + u, n))
    row_ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    row_edge = np.array([e for r in rows for e, _ in r], np.int64)
    row_var = np.array([n for r in rows for _, n in r], np.int64)
    return col_ptr, row_ptr, row_edge, row_var


def _groups(checks, row_ptr):
    """The checks split by degree: [(L, edge positions [G, L] into row_edge / row_var)]."""
    checks = np.asarray(checks, np.int64)
    deg = row_ptr[checks + 1] - row_ptr[checks]
    return [(int(L), row_ptr[checks[deg == L]][:, None] + np.arange(L)) for L in np.unique(deg) if L > 0]


def _messages(q, alg, alpha, beta, f):
    """R' [b, G, L] from q [b, G, L]."""
    L = q.shape[2]
    if L == 1:
        return np.zeros_like(q)
    if alg in (0, 1):
        a, neg = np.abs(q), q < 0
        a = np.where(np.isnan(a), np.inf, a)                             # (overflow) a NaN is skipped by the minimum and is not negative
        i1 = a.argmin(2)[..., None]                                     # the first smallest
        m1 = np.take_along_axis(a, i1, 2)
        rest = a.copy()
        np.put_along_axis(rest, i1, np.inf, 2)
        m2 = rest.min(2)[..., None]
        mag = np.where(np.arange(L) == i1, m2, m1)
        v = alpha * mag if alg == 0 else np.maximum(mag - beta, f(0))
        flip = (neg.sum(2) % 2 == 1)[..., None] != neg                   # an odd number of the others are negative
        return np.where(flip, -v, v).astype(f)
    t = np.tanh(f(0.5) * q)
    F = np.ones(q.shape[:2] + (L + 1,), f)
    S = np.ones(q.shape[:2] + (L + 1,), f)
    for l in range(L):
        F[..., l + 1] = F[..., l] * t[..., l]
    for l in range(L - 1, -1, -1):
        S[..., l] = S[..., l + 1] * t[..., l]
    p = np.clip(F[..., :L] * S[..., 1:], f(-PMAX), f(PMAX))
    return (f(2) * np.arctanh(p)).astype(f)


def decode(llr, tabs, layers=None, algorithm='min-sum', max_iter=50, alpha=0.8125, beta=0.5, dtype=np.float32):
    """llr [B, N]; tabs = ``tables(...)``; layers = (layer_ptr, layer_chk) for the layered schedule, None for flooding.  Returns a dict:
    x [B, N] uint8, viol [B], iters [B], post [B, N] ``dtype``, margin [B]."""
    with np.errstate(over='ignore', invalid='ignore'):                  # (see Overflow)
        return _decode(llr, tabs, layers, algorithm, max_iter, alpha, beta, dtype)


def _decode(llr, tabs, layers, algorithm, max_iter, alpha, beta, dtype):
    f = np.dtype(dtype).type
    alg = ALGORITHMS[algorithm]
    col_ptr, row_ptr, row_edge, row_var = tabs
    N, M, E = len(col_ptr) - 1, len(row_ptr) - 1, len(row_edge)
    llr = np.asarray(llr, np.float32)
    B = llr.shape[0]
    assert llr.shape == (B, N) and max_iter >= 1
    alpha, beta = f(np.float32(alpha)), f(np.float32(beta))
    prior = np.clip(np.where(np.isnan(llr), np.float32(0), llr), np.float32(-CLAMP), np.float32(CLAMP)).astype(f)
    T, R = prior.copy(), np.zeros((B, E), f)
    if layers is None:
        passes = [_groups(np.arange(M), row_ptr)]
    else:
        lp, lc = (np.asarray(a, np.int64) for a in layers)
        passes = [_groups(lc[lp[k]:lp[k + 1]], row_ptr) for k in range(len(lp) - 1)]
    degv = col_ptr[1:] - col_ptr[:-1]
    viol, iters = np.zeros(B, np.int64), np.zeros(B, np.int64)
    margin = np.full(B, np.inf)
    act = np.arange(B)
    for it in range(1, max_iter + 1):
        if act.size == 0:
            break
        t, r = T[act], R[act]
        for groups in passes:
            for L, pos in groups:
                ed, va = row_edge[pos], row_var[pos]
                q = t[:, va] - r[:, ed]
                out = _messages(q, alg, alpha, beta, f)
                r[:, ed] = out
                if layers is not None:
                    t[:, va] = q + out
        if layers is None:
            t = prior[act].copy()
            for u in range(int(degv.max())):
                sel = np.nonzero(degv > u)[0]
                t[:, sel] = t[:, sel] + r[:, col_ptr[sel] + u]
        T[act], R[act] = t, r
        odd = np.add.reduceat((t[:, row_var] < 0).astype(np.int64), row_ptr[:-1], axis=1) % 2
        viol[act], iters[act] = odd.sum(1), it
        margin[act] = np.minimum(margin[act], np.abs(t).min(1))
        act = act[viol[act] != 0]
    return {'x': (T < 0).astype(np.uint8), 'viol': viol, 'iters': iters, 'post': T, 'margin': margin}
