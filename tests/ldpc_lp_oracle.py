"""numpy restatement of the ADMM linear-programming LDPC decoder (csrc/ldpc_lp.hip, include/fgnn_hip_ldpc_lp.h), vectorised over the
words and over the checks of equal degree.

The steps, in the order of their operations (``dtype`` float32 restates the kernel's arithmetic; float64 is the yardstick):

  load       g[n] = llr[n] (read as f32); NaN -> 0; clamped to +-4096.  z[e] = 0.5, u[e] = 0.
  constants  amu = penalty / mu, omr = 1 - relax (the parameters are f32 values).
  variable n of degree d >= 1:  t = 0; t = t + (z[e] - u[e]) for e = col_ptr[n] ..;  x[n] = clip(((t - g[n] / mu) - amu) / (d - 2 amu), 0, 1).
             degree 0:  x[n] = (g[n] < 0).
  check m    over its edges l = 0 .. L-1 in row order:  w_l = (relax x[var_l] + omr z_l) + u_l;  z' = project(w);  u_l = w_l - z'_l;
             res = max |x[var_l] - z'_l|, dz = max |z'_l - z_l| over all edges; then z = z'.
  decision   xh[n] = x[n] > 0.5, viol = the checks of odd parity in xh.
  stop       conv = res <= eps and dz <= eps; a word stops when conv, or stop_on_codeword and viol = 0, or at max_iter.
  flags      bit 0 = conv (at the word's last iteration); bit 1 = bit 0 and min(x[n], 1 - x[n]) <= 1e-3 for every n.

project(w), the Euclidean projection onto the parity polytope by cut search:
  c = clip(w, 0, 1); f_l = w_l > 0.5; if |f| is even, f is flipped at the first l with the smallest |w_l - 0.5|;
  theta_l = +1 where f_l, else -1; p = |f| - 1;  phi(beta) = 0 + theta_0 clip(w_0 - beta theta_0, 0, 1) + theta_1 clip(...) + ...
  if phi(0) <= p: c.  Otherwise over the breakpoints b in the order (l = 0: first, second; l = 1: ...), first = w_l - 1 and second =
  w_l where f_l, first = -w_l and second = 1 - w_l elsewhere, and only those with b > 0:  v = phi(b); if v > p and b > lo: (lo, vlo) =
  (b, v); if v <= p and b < hi: (hi, vhi) = (b, v); starting from (lo, vlo) = (0, phi(0)), hi = +inf.
  beta = hi if vlo = vhi, else lo + ((vlo - p) (hi - lo)) / (vlo - vhi);  the result is clip(w - beta theta, 0, 1).

``decode`` also reports, per word, what the comparison of two precisions needs: ``margin`` (the smallest |x[n] - 0.5| at the last
iteration), ``margin_run`` (over all iterations run) and ``near`` (see ``decode``).  eps < 0 switches the residual rule off (res and dz
are never negative): the fixed-count comparisons use it.
"""
import numpy as np

CLAMP = 4096.0
INTEGRAL = 1e-3


def project(w):
    """z' [..., L] from w [..., L] (the leading axes are independent projections); the arithmetic is w's dtype."""
    f = w.dtype.type
    L = w.shape[-1]
    zero, one, half = f(0), f(1), f(0.5)
    c = np.clip(w, zero, one)
    fl = w > half
    first = np.abs(w - half).argmin(-1)[..., None]                     # the first smallest
    flip = np.zeros(w.shape, bool)
    np.put_along_axis(flip, first, True, -1)
    fl = fl ^ (flip & (fl.sum(-1) % 2 == 0)[..., None])
    theta = np.where(fl, one, -one).astype(f)
    p = (fl.sum(-1) - 1).astype(f)

    def phi(beta):
        s = np.zeros(w.shape[:-1], f)
        for l in range(L):
            s = s + theta[..., l] * np.clip(w[..., l] - beta * theta[..., l], zero, one)
        return s

    v0 = phi(np.zeros(w.shape[:-1], f))
    cut = v0 > p
    if not cut.any():
        return c
    # the search runs on the projections that need it only
    wc, tc, fc, pc = w[cut], theta[cut], fl[cut], p[cut]
    w, theta = wc, tc
    lo, vlo = np.zeros(pc.shape, f), v0[cut]
    hi, vhi = np.full(pc.shape, np.inf, f), np.zeros(pc.shape, f)
    for l in range(L):
        for b in (np.where(fc[:, l], wc[:, l] - one, -wc[:, l]), np.where(fc[:, l], wc[:, l], one - wc[:, l])):
            v = phi(b)
            up = (b > zero) & (v > pc) & (b > lo)
            dn = (b > zero) & (v <= pc) & (b < hi)
            lo, vlo = np.where(up, b, lo), np.where(up, v, vlo)
            hi, vhi = np.where(dn, b, hi), np.where(dn, v, vhi)
    same = vlo == vhi
    beta = np.where(same, hi, lo + ((vlo - pc) * (hi - lo)) / np.where(same, one, vlo - vhi))
    out = c.copy()
    out[cut] = np.clip(wc - beta[:, None] * tc, zero, one)
    return out


def _groups(row_ptr):
    """The checks split by degree: [(L, edge positions [G, L] into row_edge / row_var)]."""
    deg = row_ptr[1:] - row_ptr[:-1]
    return [(int(L), row_ptr[:-1][deg == L][:, None] + np.arange(L)) for L in np.unique(deg) if L > 0]


def min_var_degree(tabs):
    """The smallest positive variable degree of ``tables(...)`` (2 penalty / mu must stay below it)."""
    deg = np.diff(tabs[0])
    return int(deg[deg > 0].min())


def decode(llr, tabs, max_iter=200, mu=3.0, penalty=0.0, relax=1.9, eps=1e-5, stop_on_codeword=None, dtype=np.float32, tol=0.0, tol_r=0.0):
    """llr [B, N]; tabs = ``ldpc_llr_oracle.tables(...)``; ``stop_on_codeword`` None: penalty > 0.  Returns a dict: x [B, N] uint8
    (xh), soft [B, N] ``dtype`` (the final x), viol [B], iters [B], flags [B], margin [B], margin_run [B], r [B, max_iter] float64 (max(res,
    dz) per iteration run, NaN behind) and near [B] bool: at some iteration r was not zero and |r - eps| <= tol_r, or the word met the
    residual rule with some |min(x, 1 - x) - 1e-3| <= tol (a word whose stop or certificate another precision may decide
    differently).  r = 0 is exempt: it arises only from x and z that are all clipped to 0 or 1, which every precision represents
    exactly."""
    f = np.dtype(dtype).type
    col_ptr, row_ptr, row_edge, row_var = tabs
    N, M, E = len(col_ptr) - 1, len(row_ptr) - 1, len(row_edge)
    llr = np.asarray(llr, np.float32)
    B = llr.shape[0]
    assert llr.shape == (B, N) and max_iter >= 1
    soc = penalty > 0 if stop_on_codeword is None else bool(stop_on_codeword)
    mu, a, rho, eps = (f(np.float32(v)) for v in (mu, penalty, relax, eps))
    amu, omr = a / mu, f(1) - rho
    degv = col_ptr[1:] - col_ptr[:-1]
    assert not (degv > 0).any() or 2 * float(amu) < degv[degv > 0].min()
    den = np.where(degv > 0, degv.astype(f) - f(2) * amu, f(1)).astype(f)
    g = np.clip(np.where(np.isnan(llr), np.float32(0), llr), np.float32(-CLAMP), np.float32(CLAMP)).astype(f)
    Z, U, X = np.full((B, E), f(0.5)), np.zeros((B, E), f), np.zeros((B, N), f)
    groups = _groups(row_ptr)
    viol, iters, flags = np.zeros(B, np.int64), np.zeros(B, np.int64), np.zeros(B, np.int64)
    margin, margin_run, near = np.zeros(B), np.full(B, np.inf), np.zeros(B, bool)
    hist = np.full((B, max_iter), np.nan)
    act = np.arange(B)
    for it in range(1, max_iter + 1):
        if act.size == 0:
            break
        z, u, ga = Z[act], U[act], g[act]
        t = np.zeros((act.size, N), f)
        for k in range(int(degv.max())):
            sel = np.nonzero(degv > k)[0]
            t[:, sel] = t[:, sel] + (z[:, col_ptr[sel] + k] - u[:, col_ptr[sel] + k])
        x = np.clip(((t - ga / mu) - amu) / den, f(0), f(1))
        x = np.where(degv > 0, x, (ga < 0).astype(f)).astype(f)
        res, dz = np.zeros(act.size, f), np.zeros(act.size, f)
        for L, pos in groups:
            ed, va = row_edge[pos], row_var[pos]
            xv, zo = x[:, va], z[:, ed]
            w = (rho * xv + omr * zo) + u[:, ed]
            zn = project(w)
            u[:, ed] = w - zn
            z[:, ed] = zn
            res = np.maximum(res, np.abs(xv - zn).max((1, 2)))
            dz = np.maximum(dz, np.abs(zn - zo).max((1, 2)))
        Z[act], U[act], X[act] = z, u, x
        xh = x > f(0.5)
        odd = np.add.reduceat(xh[:, row_var].astype(np.int64), row_ptr[:-1], axis=1) % 2
        conv = (res <= eps) & (dz <= eps)
        frac = np.minimum(x, f(1) - x)
        integral = (frac <= f(INTEGRAL)).all(1)
        viol[act], iters[act] = odd.sum(1), it
        flags[act] = conv.astype(np.int64) + 2 * (conv & integral)
        m = np.abs(x.astype(np.float64) - 0.5).min(1)
        margin[act], margin_run[act] = m, np.minimum(margin_run[act], m)
        r = np.maximum(res, dz).astype(np.float64)
        hist[act, it - 1] = r
        near[act] |= (r > 0) & (np.abs(r - float(eps)) <= tol_r)
        near[act] |= conv & (np.abs(frac.astype(np.float64) - INTEGRAL) <= tol).any(1)
        act = act[~(conv | (soc & (odd.sum(1) == 0)))]
    return {'x': (X > f(0.5)).astype(np.uint8), 'soft': X, 'viol': viol, 'iters': iters, 'flags': flags, 'margin': margin,
            'margin_run': margin_run, 'near': near, 'r': hist}
