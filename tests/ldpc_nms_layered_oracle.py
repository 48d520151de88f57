"""Restatement of the learned min-sum LDPC decoder with a layered schedule (csrc/ldpc_nms_layered.hip,
include/fgnn_hip_ldpc_nms_layered.h).  Not a test module.

``forward``: numpy, vectorised over the batch, for a given dtype (float32 restates the kernel's arithmetic, each expression in the
header's order; float64 is the yardstick of the backward comparison):

  load         prior[n] = llr[n] (read as f32); NaN -> 0; clamped to +-4096.  T = prior, R = 0.
  iteration t  the layers in order; check m of the layer, edges l = 0..L-1 in row order: q_l = T[var_l] - R[edge_l] (the current
               values); (m1, i1) the first smallest |q|, (m2, i2) the first smallest of the rest; mag_l = m2 at l = i1, else m1;
               u_l = alpha_t[w] mag_l - beta_t[w];  R'_l = s_l max(u_l, 0), s_l negative exactly when an odd number of the other q
               are < 0;  L = 1 sends 0.  R[edge_l] = R'_l, T[var_l] = q_l + R'_l.
               After the last layer T_t = T; viol = checks of odd parity.
  w            share 'iteration': 0; 'check': m; 'edge': the edge id.

The checks of a layer share no variable, so a layer is updated at once, grouped by degree.  A NaN q (inf - inf after an overflow,
ldpc_llr_oracle's note) is skipped by the minimum and counts as non-negative.

The backward twice: ``backward`` is the header's explicit recursion on a ``forward`` result (numpy, the result's dtype);
``autograd_backward`` runs the forward again in torch float64 (two smallest by ``topk``, the other signs by a product, ``relu``,
out-of-place ``index_copy`` for R and T) and asks autograd.  tests/test_ldpc_nms_layered.py holds them against each other.
"""
import numpy as np

from ldpc_llr_oracle import CLAMP, _groups, tables  # noqa: F401  (tables: re-exported)
from ldpc_nms_oracle import SHARES, _weights, same_record, weight_count  # noqa: F401  (same_record: re-exported)


def passes(tabs, layers):
    """[(L, edge positions [G, L] into row_edge / row_var, the G checks)] in the order of the layers; the groups of one layer are
    independent of each other."""
    row_ptr = np.asarray(tabs[1], np.int64)
    lp, lc = (np.asarray(a, np.int64) for a in layers)
    out = []
    for k in range(len(lp) - 1):
        checks = lc[lp[k]:lp[k + 1]]
        deg = row_ptr[checks + 1] - row_ptr[checks]
        out += [(L, pos, checks[deg == L]) for L, pos in _groups(checks, row_ptr)]
    return out


def forward(llr, tabs, layers, alpha, beta, share, n_iter, dtype=np.float32):
    """llr [B, N]; tabs = ``tables(...)``; layers = (layer_ptr, layer_chk); alpha, beta [n_iter, W].  Every word runs all ``n_iter``
    iterations (the train mode).  Returns ``ldpc_nms_oracle.forward``'s dict: totals [n_iter, B, N] ``dtype``; x, viol (after the last
    iteration); dec_x, dec_viol, dec_iters, dec_post (the decode mode: the state after the first iteration that leaves no violated
    check, or after the last); the record m1, m2, i1, i2 [n_iter, B, M], neg and pos [n_iter, B, E] by row position; clamped [B, N];
    the arguments, 'layers' and 'passes'."""
    with np.errstate(over='ignore', invalid='ignore'):
        return _forward(llr, tabs, layers, alpha, beta, share, n_iter, dtype)


def _forward(llr, tabs, layers, alpha, beta, share, n_iter, dtype):
    f = np.dtype(dtype).type
    col_ptr, row_ptr, row_edge, row_var = tabs
    N, M, E = len(col_ptr) - 1, len(row_ptr) - 1, len(row_edge)
    llr = np.asarray(llr, np.float32)
    B = llr.shape[0]
    W = weight_count(share, tabs)
    assert llr.shape == (B, N) and np.shape(alpha) == (n_iter, W) and np.shape(beta) == (n_iter, W)
    prior32 = np.clip(np.where(np.isnan(llr), np.float32(0), llr), np.float32(-CLAMP), np.float32(CLAMP))
    clamped = ~(llr == prior32)
    T, R = prior32.astype(f), np.zeros((B, E), f)
    groups = passes(tabs, layers)
    totals = np.zeros((n_iter, B, N), f)
    m1s, m2s = np.full((n_iter, B, M), np.inf, f), np.full((n_iter, B, M), np.inf, f)
    i1s, i2s = np.full((n_iter, B, M), -1, np.int64), np.full((n_iter, B, M), -1, np.int64)
    negs, poss = np.zeros((n_iter, B, E), bool), np.zeros((n_iter, B, E), bool)
    viols = np.zeros((n_iter, B), np.int64)
    for t in range(n_iter):
        for L, pos, checks in groups:
            ed, va = row_edge[pos], row_var[pos]
            q = T[:, va] - R[:, ed]
            a, neg = np.abs(q), q < 0
            a = np.where(np.isnan(a), f(np.inf), a)
            i1 = a.argmin(2)[..., None]
            m1 = np.take_along_axis(a, i1, 2)
            negs[t][:, pos] = neg
            m1s[t][:, checks], i1s[t][:, checks] = m1[..., 0], i1[..., 0]
            out = np.zeros_like(q)                                      # L = 1 sends 0
            if L > 1:
                rest = a.copy()
                np.put_along_axis(rest, i1, np.inf, 2)
                i2 = rest.argmin(2)[..., None]
                m2 = np.take_along_axis(rest, i2, 2)
                m2s[t][:, checks], i2s[t][:, checks] = m2[..., 0], i2[..., 0]
                mag = np.where(np.arange(L) == i1, m2, m1)
                u = _weights(alpha, t, share, checks, ed, f) * mag - _weights(beta, t, share, checks, ed, f)
                o = np.maximum(u, f(0))
                flip = (neg.sum(2) % 2 == 1)[..., None] != neg          # an odd number of the others are negative
                out = np.where(flip, -o, o).astype(f)
                poss[t][:, pos] = u > 0
            R[:, ed] = out
            T[:, va] = q + out
        totals[t] = T
        viols[t] = (np.add.reduceat((T[:, row_var] < 0).astype(np.int64), row_ptr[:-1], axis=1) % 2).sum(1)
    clean = viols == 0
    stop = np.where(clean.any(0), clean.argmax(0), n_iter - 1)          # the iteration (0-based) a decode-mode word ends with
    rows = np.arange(B)
    return {'totals': totals, 'x': (T < 0).astype(np.uint8), 'viol': viols[-1], 'dec_x': (totals[stop, rows] < 0).astype(np.uint8),
            'dec_viol': viols[stop, rows], 'dec_iters': stop + 1, 'dec_post': totals[stop, rows], 'm1': m1s, 'm2': m2s, 'i1': i1s,
            'i2': i2s, 'neg': negs, 'pos': poss, 'clamped': clamped, 'tabs': tabs, 'layers': layers, 'alpha': np.asarray(alpha, np.float32),
            'beta': np.asarray(beta, np.float32), 'share': share, 'passes': groups}


def backward(fw, g_totals, words=None):
    """The header's recursion on ``fw`` = ``forward(...)`` (in its dtype), for the words ``words`` (indices or a mask; None: all):
    (g_alpha, g_beta [n_iter, W] summed over those words, g_llr [their number, N])."""
    col_ptr, row_ptr, row_edge, row_var = fw['tabs']
    f = fw['totals'].dtype.type
    n_iter, B, N = fw['totals'].shape
    E, share = len(row_edge), fw['share']
    words = np.arange(B) if words is None else np.arange(B)[words]
    g_totals = np.asarray(g_totals)[:, words].astype(f)
    m1s, m2s, i1s, i2s, negs = (fw[k][:, words] for k in ('m1', 'm2', 'i1', 'i2', 'neg'))
    ga, gb = np.zeros(fw['alpha'].shape, f), np.zeros(fw['alpha'].shape, f)
    gT, gR = np.zeros((len(words), N), f), np.zeros((len(words), E), f)
    for t in range(n_iter - 1, -1, -1):
        gT = gT + g_totals[t]
        for L, pos, checks in reversed(fw['passes']):                    # the layers backwards
            ed, va = row_edge[pos], row_var[pos]
            gq = gT[:, va]                                              # T' = q + R'
            if L > 1:
                ge = gq + gR[:, ed]
                neg = negs[t][:, pos]
                i1, i2 = i1s[t][:, checks][..., None], i2s[t][:, checks][..., None]
                at1, at2 = np.arange(L) == i1, np.arange(L) == i2
                mag = np.where(at1, m2s[t][:, checks][..., None], m1s[t][:, checks][..., None])
                al, be = _weights(fw['alpha'], t, share, checks, ed, f), _weights(fw['beta'], t, share, checks, ed, f)
                u = al * mag - be
                flip = (neg.sum(2) % 2 == 1)[..., None] != neg
                go = np.where(u > 0, np.where(flip, -ge, ge), f(0))
                if share == 'iteration':
                    ga[t, 0] += (go * mag).sum()
                    gb[t, 0] -= go.sum()
                elif share == 'check':
                    ga[t, checks] += (go * mag).sum((0, 2))
                    gb[t, checks] -= go.sum((0, 2))
                else:
                    ga[t][ed] += (go * mag).sum(0)
                    gb[t][ed] -= go.sum(0)
                gmag = go * al
                gm1 = np.where(at1, f(0), gmag).sum(2)[..., None]
                gm2 = np.where(at1, gmag, f(0)).sum(2)[..., None]
                gs = np.where(at1, gm1, np.where(at2, gm2, f(0)))
                gq = gq + np.where(neg, -gs, gs)
            gT[:, va] = gq                                              # overwrites: the check is the only reader in its layer
            gR[:, ed] = -gq
    return ga, gb, np.where(fw['clamped'][words], f(0), gT)


def torch_forward(llr, tabs, layers, alpha, beta, share, n_iter):
    """The forward in torch float64 on tensors (llr [B, N], alpha, beta [n_iter, W]; autograd follows all three): totals [n_iter, B, N]."""
    import torch
    row_edge, row_var = (torch.from_numpy(np.asarray(a, np.int64)) for a in tabs[2:])
    B, E = llr.shape[0], len(tabs[2])
    prior = torch.clamp(torch.where(torch.isnan(llr), torch.zeros_like(llr), llr), -CLAMP, CLAMP)
    T, R = prior, torch.zeros((B, E), dtype=llr.dtype)
    groups = [(L, torch.from_numpy(pos), torch.from_numpy(checks)) for L, pos, checks in passes(tabs, layers)]
    out = []
    for t in range(n_iter):
        for L, pos, checks in groups:
            if L == 1:
                continue                                                # R' = 0 = R and T' = q + 0 = T
            ed, va = row_edge[pos], row_var[pos]
            q = T[:, va] - R[:, ed]
            two, where = torch.topk(q.abs(), 2, dim=2, largest=False)
            mag = torch.where(torch.arange(L) == where[..., :1], two[..., 1:], two[..., :1])
            sgn = torch.where(q < 0, -1.0, 1.0).to(q.dtype)
            others = sgn.prod(2, keepdim=True) * sgn                     # the product of the other signs (sgn^2 = 1)
            if share == 'iteration':
                al, be = alpha[t, 0], beta[t, 0]
            elif share == 'check':
                al, be = alpha[t][checks][:, None], beta[t][checks][:, None]
            else:
                al, be = alpha[t][ed], beta[t][ed]
            new = others * torch.relu(al * mag - be)
            R = R.index_copy(1, ed.reshape(-1), new.reshape(B, -1))
            T = T.index_copy(1, va.reshape(-1), (q + new).reshape(B, -1))
        out.append(T)
    return torch.stack(out)


def autograd_backward(llr, tabs, layers, alpha, beta, share, n_iter, g_totals, words=None):
    """(g_alpha, g_beta, g_llr) as ``backward`` returns them, from torch float64 autograd over ``torch_forward``."""
    import torch
    llr = np.asarray(llr, np.float32)
    words = np.arange(len(llr)) if words is None else np.arange(len(llr))[words]
    x = torch.from_numpy(llr[words].astype(np.float64)).requires_grad_()
    a = torch.from_numpy(np.asarray(alpha, np.float32).astype(np.float64)).requires_grad_()
    b = torch.from_numpy(np.asarray(beta, np.float32).astype(np.float64)).requires_grad_()
    totals = torch_forward(x, tabs, layers, a, b, share, n_iter)
    totals.backward(torch.from_numpy(np.asarray(g_totals)[:, words].astype(np.float64)))
    return a.grad.numpy(), b.grad.numpy(), x.grad.numpy()
